"""GPU tests of the mask head's attention maps (include/attmap.h) against the float64 oracle of tests/attmap_oracle.py, run on
exactly the operands the operator received (16-bit inputs are rounded once, before both sides see them).

Forward tolerance, per element: |got - want| <= tol * (the maximum of want over the element's softmax row), tol = 1e-4 for
f32, 1e-2 for bf16 / f16 storage, 1e-10 for f64 -- the project's own bars, applied per row because a row's entries are of the
order 1 / (n * H * W).  Gradients: max|got - want| <= tol * max|want| per tensor."""
import pytest
import torch

import attmap_oracle
from test_attmap_cpu import HEADS, load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: 1e-4, torch.float64: 1e-10, torch.bfloat16: 1e-2, torch.float16: 1e-2}
DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16]
PYRAMIDS = [(12, 20), (23, 40), (45, 80), (25, 42), (50, 84), (100, 167)]


def make_inputs(B, Q, n, c, H, W, dtype, mask="quarter", gain=1.0, seed=0):
    """q ~ gain * randn, k ~ randn, rounded once to `dtype`; mask: None, "quarter" (a quarter of image 0), "ragged" (per
    image padding that cuts tiles at odd places) or "image" (all of the last image)."""
    g = torch.Generator().manual_seed(seed)
    q = (gain * torch.randn(B, Q, n * c, generator=g, dtype=torch.float64)).to(dtype)
    k = torch.randn(B, n * c, H, W, generator=g, dtype=torch.float64).to(dtype)
    m = None
    if mask is not None:
        m = torch.zeros(B, H, W, dtype=torch.bool)
        if mask == "quarter":
            m[0, H // 2:, W // 2:] = True
        elif mask == "ragged":
            for b in range(B):
                m[b, :, W - 1 - (3 * b) % (W - 1):] = True
                m[b, H - 1 - (2 * b) % (H - 1):, :] = True
        elif mask == "image":
            m[0, H // 2:, W // 2:] = True
            m[B - 1] = True
    return q, k, m


def grad_out_for(B, Q, n, H, W, dtype, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, Q, n, H, W, generator=g, dtype=torch.float64).to(dtype)


def run_op(q, k, m, n, go=None, out_dtype=None, scale=None):
    import devis_amd
    qd, kd = q.to(DEV).requires_grad_(go is not None), k.to(DEV).requires_grad_(go is not None)
    out = devis_amd.attention_maps(qd, kd, None if m is None else m.to(DEV), num_heads=n, scale=scale, out_dtype=out_dtype)
    if go is None:
        return out.detach(), None, None
    gq, gk = torch.autograd.grad(out, (qd, kd), go.to(DEV))
    return out.detach(), gq, gk


def assert_forward_close(got, want, tol, what=""):
    """per element against the row maximum; NaN rows must be NaN rows"""
    got, want = got.double().cpu().flatten(2), want.flatten(2)
    nan_rows = want.isnan().any(-1)
    assert torch.equal(got.isnan().all(-1), nan_rows) and torch.equal(got.isnan().any(-1), nan_rows), what + ": NaN rows differ"
    got, want = got[~nan_rows], want[~nan_rows]
    err = ((got - want).abs() / want.max(-1, keepdim=True).values).max() if want.numel() else torch.zeros(())
    print("%s forward: max error / row maximum = %.3e (tol %.0e)" % (what, float(err), tol))
    assert float(err) <= tol, (what, float(err))


def assert_close(got, want, tol, what):
    """max|got - want| <= tol * max|want| (tests/test_dcn_gpu.py::assert_close)"""
    err, ref = float((got.double().cpu() - want).abs().max()), float(want.abs().max())
    print("%s: max error %.3e, max |want| %.3e (tol %.0e)" % (what, err, ref, tol))
    assert err <= tol * ref, (what, err, ref)


def check_case(B, Q, n, c, H, W, dtype, mask="quarter", gain=1.0, out_dtype=None, grads=True, what=""):
    q, k, m = make_inputs(B, Q, n, c, H, W, dtype, mask, gain)
    odt = out_dtype or dtype
    go = grad_out_for(B, Q, n, H, W, odt)
    out, gq, gk = run_op(q, k, m, n, go, out_dtype)
    assert out.dtype == odt and tuple(out.shape) == (B, Q, n, H, W)
    want, wq, wk = attmap_oracle.attention_maps_with_grads(q, k, m, n, go)
    tol = TOL[dtype]
    assert_forward_close(out, want, tol, what)
    if m is not None:
        dead = m[:, None, None].expand_as(want) & ~want.isnan()
        assert float(out.double().cpu()[dead].abs().max()) == 0.0, "masked pixels must be exactly 0"
    assert gq.dtype == dtype and gk.dtype == dtype and gq.shape == q.shape and gk.shape == k.shape
    if grads:
        assert_close(gq, wq, tol, what + " grad_q")
        assert_close(gk, wk, tol, what + " grad_k")
    return out, gq, gk


# ---- numerics --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("HW", PYRAMIDS)
@pytest.mark.parametrize("Q", [1, 7, 50])
def test_f32_matches_the_oracle_at_every_level_of_both_pyramids(HW, Q):
    B = 2 if HW[0] * HW[1] > 4000 else 3
    out, _, _ = check_case(B, Q, 8, 32, HW[0], HW[1], torch.float32, what="%dx%d Q=%d" % (HW + (Q,)))
    sums = out.double().flatten(2).sum(-1)
    assert float((sums - 1).abs().max()) <= 1e-5, "every unmasked row sums to 1"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nc", [(8, 32), (4, 8), (1, 32), (2, 24)])
def test_every_dtype_and_channel_count_at_a_ragged_pixel_count(dtype, nc):
    n, c = nc
    check_case(3, 7, n, c, 13, 21, dtype, mask="ragged", what="13x21 n=%d c=%d %s" % (n, c, dtype))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float64])
def test_other_dtypes_on_a_tiled_map(dtype):
    check_case(2, 10, 8, 32, 45, 80, dtype, mask="ragged", what="45x80 %s" % dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_float32_out_beside_16_bit_inputs(dtype):
    out, _, _ = check_case(2, 7, 8, 32, 23, 40, dtype, out_dtype=torch.float32, what="%s, float32 out" % dtype)
    # the float32 maps carry no storage rounding: they meet the f32 bar against the oracle on the same 16-bit operands
    q, k, m = make_inputs(2, 7, 8, 32, 23, 40, dtype)
    assert_forward_close(out, attmap_oracle.attention_maps(q.double(), k.double(), m, 8), TOL[torch.float32], "float32 out")


@pytest.mark.parametrize("mask", [None, "ragged"])
def test_no_mask_and_masks_that_cut_a_tile(mask):
    check_case(3, 7, 8, 32, 50, 84, torch.float32, mask=mask, what="50x84 mask=%s" % mask)
    check_case(3, 7, 4, 8, 12, 20, torch.float32, mask=mask, what="12x20 mask=%s" % mask)


@pytest.mark.parametrize("HW", [(12, 20), (45, 80)])
@pytest.mark.parametrize("gain", [1.0, 8.0, 40.0])
def test_large_logits_keep_the_forward_bound(HW, gain):
    """At gain 40 logits reach +-200 and rows are one-hot: a kernel without max subtraction fails this.  The PyTorch
    formulation in float32 itself reaches 4e-5 in the gradients there, so they are asserted at gains 1 and 8 and only
    required to be finite at 40."""
    _, gq, gk = check_case(2, 7, 8, 32, HW[0], HW[1], torch.float32, gain=gain, grads=gain < 40,
                           what="%dx%d gain %g" % (HW + (gain,)))
    assert bool(gq.isfinite().all()) and bool(gk.isfinite().all())


@pytest.mark.parametrize("HW", [(13, 21), (45, 80)])
def test_a_fully_masked_image_is_nan_and_the_others_match(HW):
    q, k, m = make_inputs(3, 7, 8, 32, HW[0], HW[1], torch.float32, mask="image")
    out, _, _ = run_op(q, k, m, 8)
    assert bool(out[2].isnan().all()) and not bool(out[:2].isnan().any())
    assert_forward_close(out, attmap_oracle.attention_maps(q.double(), k.double(), m, 8), 1e-4, "masked image")


def test_no_queries_returns_an_empty_tensor():
    import devis_amd
    q, k = torch.zeros(2, 0, 32, device=DEV, requires_grad=True), torch.zeros(2, 32, 5, 6, device=DEV, requires_grad=True)
    out = devis_amd.attention_maps(q, k, num_heads=4)
    assert tuple(out.shape) == (2, 0, 4, 5, 6)
    gq, gk = torch.autograd.grad(out, (q, k), torch.zeros_like(out))
    assert tuple(gq.shape) == (2, 0, 32) and float(gk.abs().max()) == 0.0


def test_scale_and_non_contiguous_operands():
    import devis_amd
    q, k, m = make_inputs(2, 5, 4, 8, 9, 11, torch.float32)
    kt = k.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).to(DEV)       # channels-last strides
    out = devis_amd.attention_maps(q.to(DEV), kt, m.to(DEV), num_heads=4, scale=0.7)
    assert_forward_close(out, attmap_oracle.attention_maps(q.double(), k.double(), m, 4, scale=0.7), 1e-4, "scale 0.7")


# ---- module ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["attmap_masked", "attmap_nomask", "attmap_nobias"])
def test_module_matches_the_reference_fixture(name):
    from devis_amd.modules import MultiScaleMHAttentionMap
    d, levels, state, masks = load_fixture(name)
    m = MultiScaleMHAttentionMap(8, 32, HEADS, levels, bias="q_linear.bias" in state)
    m.load_state_dict(state, strict=True)
    m = m.to(DEV, torch.float32)
    q = d["q"].float().to(DEV).requires_grad_(True)
    # DeVIS hands the module views of the transformer's memory: channels-last strides here
    ks = [d["k/%d" % i].float().to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
          for i in range(levels)]
    outs = m(q, ks, None if masks is None else [mk.to(DEV) for mk in masks])
    params = dict(m.named_parameters())
    grads = torch.autograd.grad(outs, [q] + ks + list(params.values()), [d["grad_out/%d" % i].float().to(DEV) for i in range(levels)])
    for i, o in enumerate(outs):
        assert_forward_close(o.detach(), d["out/%d" % i], 1e-4, "%s level %d" % (name, i))
    want = [d["grad/q"]] + [d["grad/k/%d" % i] for i in range(levels)] + [d["grad/state/" + n] for n in params]
    names = ["q"] + ["k/%d" % i for i in range(levels)] + list(params)
    for g, w, nm in zip(grads, want, names):
        assert_close(g, w, 1e-4, "%s grad %s" % (name, nm))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_autocast_gives_float32_maps_and_float32_parameter_gradients(dtype):
    from devis_amd.modules import MultiScaleMHAttentionMap
    d, levels, state, masks = load_fixture("attmap_masked")
    m = MultiScaleMHAttentionMap(8, 32, HEADS, levels)
    m.load_state_dict(state, strict=True)
    m = m.to(DEV, torch.float32)
    q = d["q"].float().to(DEV).requires_grad_(True)
    ks = [d["k/%d" % i].float().to(DEV) for i in range(levels)]
    with torch.autocast("cuda", dtype=dtype):
        outs = m(q, ks, [mk.to(DEV) for mk in masks])
    assert all(o.dtype == torch.float32 for o in outs)
    torch.autograd.backward(outs, [d["grad_out/%d" % i].float().to(DEV) for i in range(levels)])
    assert q.grad.dtype == torch.float32
    for name, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(p.grad.isfinite().all()), name


# ---- reproducibility, partial backward, overwrite contract -----------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_launches_give_identical_bits_also_in_deterministic_mode(dtype):
    import warnings
    q, k, m = make_inputs(3, 10, 8, 32, 45, 80, dtype, mask="ragged")
    go = grad_out_for(3, 10, 8, 45, 80, dtype)
    first = run_op(q, k, m, 8, go)
    for _ in range(2):
        for a, b in zip(first, run_op(q, k, m, 8, go)):
            assert torch.equal(a, b)
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            again = run_op(q, k, m, 8, go)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)
    assert torch.equal(first[0], again[0])


@pytest.mark.parametrize("HW", [(13, 21), (50, 84)])
def test_each_gradient_alone_equals_the_full_backward_bit_for_bit(HW):
    import devis_amd
    B, Q, n = 2, 7, 8
    q, k, m = make_inputs(B, Q, n, 32, HW[0], HW[1], torch.float32)
    go = grad_out_for(B, Q, n, HW[0], HW[1], torch.float32).to(DEV)
    _, gq, gk = run_op(q, k, m, n, go)
    for need_q in (True, False):
        qd, kd = q.to(DEV).requires_grad_(need_q), k.to(DEV).requires_grad_(not need_q)
        out = devis_amd.attention_maps(qd, kd, m.to(DEV), num_heads=n)
        out.backward(go)
        if need_q:
            assert kd.grad is None and torch.equal(qd.grad, gq)
        else:
            assert qd.grad is None and torch.equal(kd.grad, gk)


def test_output_and_workspace_prefilled_with_nan_are_fully_overwritten(monkeypatch):
    """torch.empty is replaced by a NaN-filling one inside the host code: every buffer the operator allocates (out, dl, the
    partials' workspace) is then fully overwritten, or the results would carry the NaNs."""
    from devis_amd.functions import attention_maps as A
    real = torch.empty

    def nan_empty(*a, **kw):
        t = real(*a, **kw)
        if t.dtype == torch.uint8:
            t.fill_(255)        # all-ones bytes: NaN as floats of any width
        elif t.is_floating_point():
            t.fill_(float("nan"))
        return t

    shim = type("T", (), {"__getattr__": lambda self, name: nan_empty if name == "empty" else getattr(torch, name)})()
    monkeypatch.setattr(A, "torch", shim)
    for HW in ((13, 21), (45, 80), (50, 84)):
        check_case(2, 9, 8, 32, HW[0], HW[1], torch.float32, mask="ragged", what="NaN-filled %dx%d" % HW)
    check_case(2, 9, 8, 32, 13, 21, torch.bfloat16, mask="ragged", out_dtype=torch.float32, what="NaN-filled bf16")


# ---- other execution modes -------------------------------------------------------------------------------------------

def test_gradcheck_on_the_f64_path():
    import devis_amd
    q, k, m = make_inputs(2, 3, 2, 4, 5, 7, torch.float64)
    qd, kd, md = q.to(DEV).requires_grad_(True), k.to(DEV).requires_grad_(True), m.to(DEV)
    assert torch.autograd.gradcheck(lambda q, k: devis_amd.attention_maps(q, k, md, num_heads=2), (qd, kd))
    from devis_amd import ops
    assert torch.autograd.gradcheck(lambda q, k: ops.attention_maps_op(q, k, md, 2, 0.5), (qd, kd))


def test_compile_fullgraph_equals_eager_also_with_dynamic_shapes():
    import devis_amd
    fn = lambda q, k, m: devis_amd.attention_maps(q, k, m, num_heads=8)      # noqa: E731
    compiled = torch.compile(fn, fullgraph=True)
    for Q, H, W in ((7, 13, 21), (10, 23, 40), (3, 12, 20)):
        q, k, m = make_inputs(2, Q, 8, 32, H, W, torch.float32)
        go = grad_out_for(2, Q, 8, H, W, torch.float32).to(DEV)
        want = run_op(q, k, m, 8, go)
        qd, kd, md = q.to(DEV).requires_grad_(True), k.to(DEV).requires_grad_(True), m.to(DEV)
        torch._dynamo.mark_dynamic(qd, 1)       # Q, H and W are dynamic: one graph serves the three shapes
        for t, dims in ((kd, (2, 3)), (md, (1, 2))):
            for dim in dims:
                torch._dynamo.mark_dynamic(t, dim)
        out = compiled(qd, kd, md)
        gq, gk = torch.autograd.grad(out, (qd, kd), go)
        assert torch.equal(out, want[0]) and torch.equal(gq, want[1]) and torch.equal(gk, want[2])


def test_hip_graph_replay_with_changed_inputs_gives_the_changed_result():
    import devis_amd
    q, k, m = make_inputs(2, 7, 8, 32, 23, 40, torch.float32)
    sq, sk, sm = q.to(DEV).clone(), k.to(DEV).clone(), m.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        devis_amd.attention_maps(sq, sk, sm, num_heads=8)      # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = devis_amd.attention_maps(sq, sk, sm, num_heads=8)
    q2, k2, _ = make_inputs(2, 7, 8, 32, 23, 40, torch.float32, seed=5)
    sq.copy_(q2), sk.copy_(k2)
    graph.replay()
    torch.cuda.synchronize()
    want = devis_amd.attention_maps(q2.to(DEV), k2.to(DEV), sm, num_heads=8)
    assert torch.equal(out, want)
    assert_forward_close(out, attmap_oracle.attention_maps(q2.double(), k2.double(), m, 8), 1e-4, "graph replay")
