"""GPU tests of the mask loss (include/maskloss.h) against the float64 oracle of tests/maskloss_oracle.py, run on exactly the
logits the operator received (16-bit logits are rounded once, before both sides see them; the oracle evaluates the taps in
float32 as the kernels do, in float64 for float64 logits).

Tolerance, per tensor (focal [N], dice [N], grad_src): max|got - want| <= tol * max|want|, tol = 1e-4 for f32, 1e-2 for
bf16 / f16 storage, 1e-10 for f64 -- the project's own bars (tests/test_attmap_gpu.py)."""
import warnings

import pytest
import torch
import torch.nn.functional as F

import maskloss_oracle
from test_attmap_gpu import TOL, assert_close
from test_maskloss_cpu import FIXTURES, StandInCriterion, load_fixture, stand_in_case, stock_losses

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16]
F64 = torch.float64


def make_case(N, hw, HW, dtype=torch.float32, seed=0, gain=2.5, fill=0.5):
    """(src [N, h, w] ~ gain * randn rounded once to `dtype`, bool target [N, H, W] with about `fill` ones)."""
    g = torch.Generator().manual_seed(seed)
    src = (gain * torch.randn(N, *hw, generator=g, dtype=F64)).to(dtype)
    return src, torch.rand(N, *HW, generator=g) < fill


def grads_for(N, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, generator=g, dtype=F64), torch.randn(N, generator=g, dtype=F64)


def arith_of(dtype):
    return F64 if dtype == F64 else torch.float32


def run_op(src, target, alpha=0.25, gamma=2.0, grads=None):
    """(focal, dice, grad_src or None) of the operator, on the device."""
    import devis_amd
    s = src.to(DEV).requires_grad_(grads is not None)
    t = target if target.is_cuda else target.to(DEV)
    focal, dice = devis_amd.mask_loss_terms(s, t, alpha, gamma)
    if grads is None:
        return focal.detach(), dice.detach(), None
    gs, = torch.autograd.grad([focal, dice], s, [g.to(DEV, focal.dtype) for g in grads])
    return focal.detach(), dice.detach(), gs


def check_case(src, target, alpha=0.25, gamma=2.0, what="", tol=None):
    dtype = src.dtype
    grads = grads_for(src.shape[0])
    focal, dice, gs = run_op(src, target, alpha, gamma, grads)
    # the gradients the operator saw are rounded to its arithmetic type
    seen = tuple(g.to(focal.dtype).double() for g in grads)
    wf, wd, wg = maskloss_oracle.mask_loss_terms(src.double().reshape(src.shape[0], *src.shape[-2:]), target.cpu(), alpha, gamma,
                                                 arith_of(dtype), grads=seen)
    assert focal.dtype == dice.dtype == arith_of(dtype) and gs.dtype == dtype and gs.shape == src.shape
    tol = tol or TOL[dtype]
    # the loss terms are sums in the arithmetic type whatever the storage type: 16-bit logits do not loosen them
    loss_tol = min(tol, 1e-4) if dtype != F64 else tol
    assert_close(focal, wf, loss_tol, what + " focal")
    assert_close(dice, wd, loss_tol, what + " dice")
    assert_close(gs.reshape(wg.shape), wg, tol, what + " grad_src")
    return focal, dice, gs


# ---- fixtures and dtypes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_in_float64_equal_the_reference(name):
    import devis_amd
    d = load_fixture(name)
    src = d["src"].to(DEV).requires_grad_(True)
    out = devis_amd.mask_losses(src, d["target"].to(DEV), d["num_boxes"], alpha=d["alpha"])
    grad, = torch.autograd.grad(out["loss_mask"] + out["loss_dice"], src)
    assert_close(out["loss_mask"], d["loss_mask"], 1e-10, name + " loss_mask")
    assert_close(out["loss_dice"], d["loss_dice"], 1e-10, name + " loss_dice")
    assert_close(grad, d["grad_src"], 1e-10, name + " grad_src")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_in_every_dtype_equal_the_oracle(name, dtype):
    d = load_fixture(name)
    check_case(d["src"].to(dtype), d["target"], d["alpha"], what="%s %s" % (name, dtype))


def test_target_kinds_give_the_same_bits_and_a_soft_target_equals_the_oracle():
    for dtype in (torch.float32, torch.bfloat16, torch.float64):
        src, target = make_case(3, (9, 11), (30, 41), dtype)
        grads = grads_for(3)
        want = run_op(src, target, grads=grads)
        kinds = [target.to(torch.uint8) * 7, target.to(dtype)] + ([target.float()] if dtype != F64 else [])
        for t in kinds:
            got = run_op(src, t, grads=grads)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (dtype, t.dtype)
    g = torch.Generator().manual_seed(3)
    src, _ = make_case(3, (9, 11), (30, 41))
    for soft in (torch.rand(3, 30, 41, generator=g), torch.rand(3, 30, 41, generator=g, dtype=F64).to(torch.bfloat16).float()):
        check_case(src, soft, what="soft target")
    srch, _ = make_case(3, (9, 11), (30, 41), torch.float16)
    check_case(srch, torch.rand(3, 30, 41, generator=g), what="soft float32 target beside float16 logits")


# ---- the tap rule ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [((14, 14), (46, 46)), ((12, 12), (45, 45)), ((14, 12), (46, 45)), ((13, 17), (13, 17))])
def test_tap_rule(sizes):
    """tests/test_maskloss_cpu.py::test_a_wrong_tap_rule_is_far_outside_the_tolerance shows that align_corners=True or an
    integer ratio misses 1e-4 by more than a factor of ten at these sizes."""
    src, target = make_case(3, sizes[0], sizes[1], torch.float32, seed=7)
    check_case(src, target, what="%s -> %s" % sizes)
    if sizes[0] == sizes[1]:        # the identity resamples nothing: the stock losses on the logits themselves
        focal, dice, _ = run_op(src, target)
        x, t = src.double().flatten(1), target.double().flatten(1)
        p = x.sigmoid()
        want = (F.binary_cross_entropy_with_logits(x, t, reduction="none") * (1 - (p * t + (1 - p) * (1 - t))) ** 2
                * (0.25 * t + 0.75 * (1 - t))).mean(1)
        assert_close(focal, want, 1e-4, "identity focal")


# ---- tiling boundaries -----------------------------------------------------------------------------------------------

def _tiles():
    from devis_amd import _maskloss
    return tuple(_maskloss.tile(k) for k in (_maskloss.TILE_FWD_PIXELS, _maskloss.TILE_FWD_SRC, _maskloss.TILE_BWD_ROWS,
                                             _maskloss.TILE_BWD_COLS, _maskloss.TILE_BWD_CHUNK))


def test_forward_tiles_at_one_tile_one_more_one_less_and_two_plus_one():
    fwd = _tiles()[0]
    assert fwd == 4096
    for H, W in ((64, 64), (63, 65), (17, 241), (3, 2731)):        # P = one tile, one less, one more, two tiles + 1
        assert H * W in (fwd, fwd - 1, fwd + 1, 2 * fwd + 1)
        src, target = make_case(2, (9, 13), (H, W), seed=H)
        check_case(src, target, what="P = %d" % (H * W))


def test_backward_tiles_at_one_tile_one_more_one_less_and_two_plus_one():
    _, _, rows, cols, chunk = _tiles()
    for h, w in ((rows, cols), (rows - 1, cols - 1), (rows + 1, cols + 1), (2 * rows + 1, 2 * cols + 1), (rows, cols + 1)):
        src, target = make_case(2, (h, w), (3 * h + 1, 2 * w + 3), seed=h * w)
        check_case(src, target, what="h x w = %d x %d" % (h, w))
    # a tile whose destination region is more than one chunk: by rows (4.5x up), and by columns (one source column)
    src, target = make_case(1, (rows, cols), (36, 144), seed=2)
    assert 36 * 144 > chunk
    check_case(src, target, what="two row chunks")
    src, target = make_case(2, (2, 1), (2, chunk + 905), seed=3)
    check_case(src, target, what="column chunks")


def test_a_tile_whose_source_rows_do_not_fit_the_lds_reads_memory():
    cap = _tiles()[1]
    src, target = make_case(2, (70, 70), (3, 3), seed=4)
    assert 70 * 70 > cap
    check_case(src, target, what="70x70 -> 3x3")


@pytest.mark.parametrize("W", [15, 16, 17])
def test_widths_around_the_16_pixel_vector_path(W):
    src, target = make_case(3, (5, 6), (19, W), seed=W)
    check_case(src, target, what="W = %d" % W)


def test_a_target_view_at_an_odd_byte_offset_gives_the_bits_of_the_aligned_one():
    src, target = make_case(3, (8, 8), (32, 32))
    grads = grads_for(3)
    want = run_op(src, target, grads=grads)
    buf = torch.zeros(3 * 32 * 32 + 16, dtype=torch.bool, device=DEV)
    view = buf[1:1 + 3 * 32 * 32].view(3, 32, 32)
    view.copy_(target)
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    got = run_op(src, view, grads=grads)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    strided = torch.zeros(3, 32, 64, dtype=torch.bool, device=DEV)[:, :, ::2]       # not dense: made dense
    strided.copy_(target)
    got = run_op(src, strided, grads=grads)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    check_case(src, target, what="aligned")


# ---- degenerate maps and values --------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [((1, 9), (4, 30)), ((9, 1), (30, 4)), ((1, 1), (5, 7)), ((26, 22), (13, 11)), ((1, 1), (1, 1))])
def test_degenerate_maps(sizes):
    for dtype in (torch.float32, torch.float64):
        src, target = make_case(3, sizes[0], sizes[1], dtype, seed=11)
        check_case(src, target, what="%s -> %s %s" % (sizes + (dtype,)))


@pytest.mark.parametrize("dtype,big", [(torch.float32, 80.0), (torch.float16, 6.0e4)])
def test_saturated_logits_give_finite_losses_and_gradients(dtype, big):
    # instances: +big / -big logits against all-0 and all-1 targets, and one mixed
    src = torch.full((5, 6, 7), big, dtype=F64)
    src[2:4] = -big
    src[4, :, ::2] = -big
    target = torch.zeros(5, 20, 23, dtype=torch.bool)
    target[1], target[3] = True, True
    target[4, :10] = True
    focal, dice, gs = check_case(src.to(dtype), target, what="saturated %s" % dtype)
    assert bool(focal.isfinite().all()) and bool(dice.isfinite().all()) and bool(gs.float().isfinite().all())


@pytest.mark.parametrize("gamma", [0.0, 1.0, 2.0, 3.0])
@pytest.mark.parametrize("alpha", [0.25, -1.0])
def test_alpha_and_gamma(alpha, gamma):
    src, target = make_case(3, (7, 9), (27, 35), seed=5)
    check_case(src, target, alpha, gamma, what="alpha %s gamma %s" % (alpha, gamma))
    src, target = make_case(2, (7, 9), (27, 35), F64, seed=5)
    check_case(src, target, alpha, gamma, what="f64 alpha %s gamma %s" % (alpha, gamma))


def test_no_instance_gives_empty_vectors_and_zero_losses_and_launches_nothing(monkeypatch):
    import devis_amd
    from devis_amd import _maskloss

    def no_launch(*a, **k):
        raise AssertionError("a kernel call was made")

    monkeypatch.setattr(_maskloss, "forward", no_launch)
    monkeypatch.setattr(_maskloss, "backward", no_launch)
    src = torch.zeros(0, 6, 7, device=DEV, requires_grad=True)
    target = torch.zeros(0, 20, 23, dtype=torch.bool, device=DEV)
    focal, dice = devis_amd.mask_loss_terms(src, target)
    assert tuple(focal.shape) == tuple(dice.shape) == (0,) and focal.dtype == torch.float32
    out = devis_amd.mask_losses(src, target, 2.0)
    assert float(out["loss_mask"]) == 0.0 and float(out["loss_dice"]) == 0.0
    grad, = torch.autograd.grad(out["loss_mask"] + out["loss_dice"], src)
    assert tuple(grad.shape) == (0, 6, 7)


def test_four_dimensional_logits():
    src, target = make_case(3, (7, 9), (27, 35))
    grads = grads_for(3)
    want = run_op(src, target, grads=grads)
    got = run_op(src[:, None], target, grads=grads)
    assert tuple(got[2].shape) == (3, 1, 7, 9)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2][:, 0], want[2])


# ---- reproducibility -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_runs_give_identical_bits_also_in_deterministic_mode(dtype):
    src, target = make_case(4, (12, 20), (45, 96), dtype)       # two forward tiles, two backward tiles
    grads = grads_for(4)
    first = run_op(src, target, grads=grads)
    for _ in range(2):
        assert all(torch.equal(a, b) for a, b in zip(run_op(src, target, grads=grads), first))
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            again = run_op(src, target, grads=grads)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)
    assert all(torch.equal(a, b) for a, b in zip(again, first))


def test_an_instance_has_the_same_bits_alone_and_in_a_batch_of_five():
    src, target = make_case(5, (12, 20), (45, 96))
    grads = grads_for(5)
    focal, dice, gs = run_op(src, target, grads=grads)
    f1, d1, g1 = run_op(src[3:4], target[3:4], grads=(grads[0][3:4], grads[1][3:4]))
    assert torch.equal(f1, focal[3:4]) and torch.equal(d1, dice[3:4]) and torch.equal(g1, gs[3:4])


# ---- memory ----------------------------------------------------------------------------------------------------------

def test_forward_and_backward_allocate_no_full_resolution_float_tensor():
    import devis_amd
    N, H, W = 8, 256, 256
    src, target = make_case(N, (32, 32), (H, W))
    src, target = src.to(DEV).requires_grad_(True), target.to(DEV)
    full = N * H * W * 4

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss = fn()
        grad, = torch.autograd.grad(loss, src)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, loss.detach(), grad

    def fused():
        out = devis_amd.mask_losses(src, target, 4.0)
        return out["loss_mask"] + out["loss_dice"]

    def stock():
        lm, ld = stock_losses(src, target, 4.0)
        return lm + ld

    fused()         # (the library and the allocator are warm before anything is measured)
    ours, loss, grad = peak(fused)
    theirs, loss2, grad2 = peak(stock)
    print("peak bytes over forward + backward: fused %d, stock %d, one full-resolution float tensor %d" % (ours, theirs, full))
    assert ours < full
    assert theirs > 3 * full            # the measurement sees such tensors when they exist
    assert_close(loss, loss2.double().cpu(), 1e-4, "loss against the stock formulation in float32")
    assert_close(grad, grad2.double().cpu(), 1e-4, "grad against the stock formulation in float32")


# ---- the public pair, the drop-in, compile and graphs -----------------------------------------------------------------

@pytest.mark.parametrize("num_boxes", [3.0, "tensor"])
def test_mask_losses_equal_the_stock_formulation_in_float64(num_boxes):
    import devis_amd
    src, target = make_case(4, (12, 20), (45, 80), seed=9)
    nb = torch.tensor(3.0, device=DEV) if num_boxes == "tensor" else num_boxes
    s = src.to(DEV).requires_grad_(True)
    out = devis_amd.mask_losses(s, target.to(DEV), nb)
    assert sorted(out) == ["loss_dice", "loss_mask"] and out["loss_mask"].dim() == 0 and out["loss_mask"].dtype == torch.float32
    grad, = torch.autograd.grad(out["loss_mask"] + out["loss_dice"], s)
    ref = src.double().requires_grad_(True)
    lm, ld = stock_losses(ref, target, 3.0)
    want, = torch.autograd.grad(lm + ld, ref)
    assert_close(out["loss_mask"], lm.detach(), 1e-4, "loss_mask")
    assert_close(out["loss_dice"], ld.detach(), 1e-4, "loss_dice")
    assert_close(grad, want, 1e-4, "grad_src")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        cast = devis_amd.mask_losses(s, target.to(DEV), nb)
    assert cast["loss_mask"].dtype == torch.float32 and torch.equal(cast["loss_mask"], out["loss_mask"])
    assert torch.equal(cast["loss_dice"], out["loss_dice"])


@pytest.mark.parametrize("form", ["image", "devis", "devis_empty"])
def test_loss_masks_equals_the_stock_formulation(form):
    from devis_amd import argument_builders
    outputs, targets, indices, want_s, want_t = stand_in_case(form, DEV)
    outputs["pred_masks"].requires_grad_(True)
    out = argument_builders.loss_masks(StandInCriterion(), outputs, targets, indices, 2.0)
    grad, = torch.autograd.grad(out["loss_mask"] + out["loss_dice"], outputs["pred_masks"])
    if form == "devis_empty":
        assert float(out["loss_mask"]) == 0.0 and float(out["loss_dice"]) == 0.0 and float(grad.abs().max()) == 0.0
        return
    ref = want_s.double().requires_grad_(True)
    lm, ld = stock_losses(ref, want_t, 2.0)
    want, = torch.autograd.grad(lm + ld, ref)
    assert_close(out["loss_mask"], lm.detach(), 1e-4, form + " loss_mask")
    assert_close(out["loss_dice"], ld.detach(), 1e-4, form + " loss_dice")
    assert_close(grad.reshape(want.shape), want, 1e-4, form + " grad")


def test_compile_fullgraph_equals_eager_also_with_dynamic_shapes():
    """The operator's own outputs and gradient are bitwise those of eager.  The two scalars of mask_losses are a sum and a
    division that the compiler generates itself: they, and the gradient that flows through them, are compared at 1e-6, a few
    float32 roundings of at most six terms."""
    import devis_amd

    def terms(s, t):
        return devis_amd.mask_loss_terms(s, t)

    def losses(s, t):
        out = devis_amd.mask_losses(s, t, 3.0)
        return out["loss_mask"], out["loss_dice"]

    compiled_terms, compiled_losses = torch.compile(terms, fullgraph=True), torch.compile(losses, fullgraph=True)
    for N, hw, HW in ((4, (6, 10), (24, 40)), (6, (7, 9), (27, 35)), (3, (12, 20), (45, 80))):
        src, target = make_case(N, hw, HW, seed=N)
        gf, gd = (g.to(DEV, torch.float32) for g in grads_for(N))
        t = target.to(DEV)

        def leaf(dynamic):
            s = src.to(DEV).requires_grad_(True)
            if dynamic:     # the map sizes are marked; the changing N goes dynamic by itself on the second call
                for tensor in (s, t):
                    for dim in (1, 2):
                        torch._dynamo.mark_dynamic(tensor, dim)
            return s

        s = leaf(False)
        want = terms(s, t)
        want_grad, = torch.autograd.grad(list(want), s, [gf, gd])
        s = leaf(False)
        want_losses = losses(s, t)
        want_whole, = torch.autograd.grad(want_losses[0] + want_losses[1], s)
        s = leaf(True)
        got = compiled_terms(s, t)
        grad, = torch.autograd.grad(list(got), s, [gf, gd])
        print("N = %d: terms differ by %.3e, %.3e, gradient by %.3e" % (N, float((got[0] - want[0]).abs().max()),
              float((got[1] - want[1]).abs().max()), float((grad - want_grad).abs().max())))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(grad, want_grad)
        s = leaf(True)
        got_losses = compiled_losses(s, t)
        whole, = torch.autograd.grad(got_losses[0] + got_losses[1], s)
        assert_close(got_losses[0].detach(), want_losses[0].detach().double().cpu(), 1e-6, "compiled loss_mask")
        assert_close(got_losses[1].detach(), want_losses[1].detach().double().cpu(), 1e-6, "compiled loss_dice")
        assert_close(whole, want_whole.double().cpu(), 1e-6, "compiled gradient of the two losses")


def test_hip_graph_replay_with_changed_inputs_gives_the_changed_result():
    import devis_amd
    src, target = make_case(4, (12, 20), (45, 96))
    s, t = src.to(DEV).clone(), target.to(DEV).clone()
    call = lambda a, b: torch.stack(devis_amd.mask_loss_terms(a, b))      # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(s, t)          # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(s, t)
    src2, target2 = make_case(4, (12, 20), (45, 96), seed=5)
    s.copy_(src2)
    t.copy_(target2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, call(src2.to(DEV), target2.to(DEV)))
    wf, wd = maskloss_oracle.mask_loss_terms(src2.double(), target2)
    assert_close(out[0], wf, 1e-4, "graph replay focal")
    assert_close(out[1], wd, 1e-4, "graph replay dice")
