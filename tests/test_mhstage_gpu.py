"""GPU tests of the mask-head stage (include/mhstage.h) against the float64 oracle of tests/mhstage_oracle.py, run on exactly
the operands the operator received (16-bit inputs are rounded once, before both sides see them).

Tolerances are the project's own (tests/test_attmap_gpu.py TOL): max|got - want| <= tol * max|want| per tensor, tol = 1e-4
for f32, 1e-2 for bf16 / f16 storage, 1e-10 for f64.

The ReLU gate: an element whose pre-activation z is within rounding of 0 may be gated differently in fp32 and fp64, and its
gradient then differs by a whole term.  The gradient comparisons give the oracle the gate z64 > 0, except for the elements
with |z64| <= 1e-5 * max|z64| (1e-12 for f64), which take the device's gate, read as out > 0 from a plain float32-out call on
the same x.  Such elements must be at most 1 in 1000 of x; the count is printed."""
import warnings

import pytest
import torch
import torch.nn.functional as F

import mhstage_oracle
from test_attmap_gpu import TOL, DTYPES, assert_close
from test_mhstage_cpu import EXPANDS, load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("x", "weight", "bias", "skip", "extra")
# every stage kind of the real head: (N, F, C, G, E, (h, w), (H, W)); F = 0: no skip
STAGES = [(6, 0, 264, 8, 0, (5, 7), (5, 7)), (6, 3, 128, 8, 8, (5, 7), (9, 14)), (6, 3, 64, 8, 8, (6, 10), (12, 20)),
          (4, 2, 32, 8, 0, (7, 5), (14, 10)), (4, 0, 16, 8, 0, (9, 11), (9, 11))]


def index_for(kind, N, F, dtype=torch.int64, seed=3):
    if kind is None:
        return None
    if kind == "repeat":
        idx = torch.arange(F).repeat(N // F)
    elif kind == "interleaved":
        idx = torch.arange(F).repeat_interleave(N // F)
    elif kind == "ragged":          # the first image three times, the last takes the rest; the ones between once
        idx = torch.cat([torch.zeros(3), torch.arange(1, F - 1), torch.full((N - 3 - (F - 2),), F - 1)])
    elif kind == "unused":          # image 1 of the F is used by no instance
        idx = torch.where(torch.arange(N) < N // 2, 0, F - 1)
    else:
        idx = torch.randperm(F, generator=torch.Generator().manual_seed(seed))
    assert idx.numel() == N
    return idx.to(dtype)


def make_case(N, F, C, G, E, hw, HW, dtype, kind="repeat", index_dtype=torch.int64, param_dtype=None, extra_dtype=None, seed=0):
    """x = 1.5 * randn + 0.3, weight = 0.5 * randn + 1, bias = 0.3 * randn (the issue's inputs), rounded once."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    d = {"x": (1.5 * rnd(N, C, *hw) + 0.3).to(dtype), "weight": (0.5 * rnd(C) + 1).to(param_dtype or dtype),
         "bias": (0.3 * rnd(C)).to(param_dtype or dtype), "skip": None, "extra": None, "index": None, "G": G}
    if F:
        d["skip"] = rnd(F, C, *HW).to(dtype)
        d["index"] = index_for(kind, N, F, index_dtype)
    if E:
        d["extra"] = (0.5 * rnd(N, E, *HW)).to(extra_dtype or dtype)
    return d


def grad_out_for(d, dtype, seed=1):
    N, C = d["x"].shape[:2]
    E = 0 if d["extra"] is None else d["extra"].shape[1]
    HW = d["skip"].shape[-2:] if d["skip"] is not None else d["extra"].shape[-2:] if d["extra"] is not None else d["x"].shape[-2:]
    return torch.randn(N, C + E, *HW, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype)


def run_op(d, go=None, out_dtype=None, need=NAMES):
    """(out, {name: gradient}) of the operator on the GPU."""
    import devis_amd
    t = {k: (None if d[k] is None else d[k].to(DEV).requires_grad_(go is not None and k in need)) for k in NAMES}
    idx = None if d["index"] is None else d["index"].to(DEV)
    out = devis_amd.mask_head_stage(t["x"], d["G"], t["weight"], t["bias"], skip=t["skip"], skip_index=idx, extra=t["extra"],
                                    out_dtype=out_dtype)
    if go is None:
        return out.detach(), {}
    leaves = {k: v for k, v in t.items() if v is not None and v.requires_grad}
    grads = torch.autograd.grad(out, list(leaves.values()), go if go.is_cuda else go.to(DEV))
    return out.detach(), dict(zip(leaves, grads))


def gate_for(d, dtype):
    """The oracle's gate for case d (module docstring); asserts the share of near-zero pre-activations."""
    import devis_amd
    z64 = mhstage_oracle.pre_activation(d["x"], d["G"], d["weight"], d["bias"])
    wide = torch.float32 if dtype in (torch.bfloat16, torch.float16) else None
    plain = devis_amd.mask_head_stage(d["x"].to(DEV), d["G"], d["weight"].to(DEV), d["bias"].to(DEV), out_dtype=wide)
    gate, near = mhstage_oracle.device_gate(z64, plain, 1e-12 if dtype == torch.float64 else 1e-5)
    print("pre-activations within rounding of zero: %d of %d" % (near, z64.numel()))
    assert near * 1000 <= z64.numel()
    return gate


def check_case(d, dtype, out_dtype=None, what=""):
    odt = out_dtype or dtype
    go = grad_out_for(d, odt)
    out, grads = run_op(d, go, out_dtype)
    N, C, h, w = d["x"].shape
    assert out.dtype == odt and tuple(out.shape) == tuple(go.shape)
    assert out.is_contiguous(memory_format=torch.channels_last)
    tol = TOL[dtype]
    want = mhstage_oracle.mask_head_stage(d["x"], d["G"], d["weight"], d["bias"], 1e-5, d["skip"], d["index"], d["extra"])
    assert_close(out, want, tol, what + " out")
    _, wg = mhstage_oracle.with_grads(d["x"], d["G"], d["weight"], d["bias"], go, 1e-5, d["skip"], d["index"], d["extra"],
                                      gate_for(d, dtype))
    assert sorted(grads) == sorted(wg)
    for name, g in grads.items():
        assert g.dtype == d[name].dtype and g.shape == d[name].shape, name
        assert_close(g, wg[name], tol, "%s grad_%s" % (what, name))
    return out, grads


# ---- numerics --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("stage", STAGES)
def test_every_stage_kind_of_the_head_in_every_dtype(stage, dtype):
    check_case(make_case(*stage, dtype), dtype, what="%s %s" % (stage, dtype))


@pytest.mark.parametrize("case", [(4, 2, 16, 8, 0, (14, 3), (46, 5)), (2, 2, 8, 2, 0, (26, 2), (22, 3))])
def test_index_rule_is_bitwise_f_interpolate(case):
    """The resized stage against F.interpolate (on the GPU) of the same stage without resizing, bit for bit, in f64: both
    evaluate one expression per element, so only the nearest-neighbour index differs.  14 -> 46 is the smallest pair on
    which the integer rule (d * h) // H fails (d = 23); 26 -> 22 downsamples."""
    import devis_amd
    N, F_, C, G, E, hw, HW = case
    d = make_case(N, N, C, G, E, hw, HW, torch.float64, kind=None)
    x, wt, b = d["x"].to(DEV), d["weight"].to(DEV), d["bias"].to(DEV)
    plain = devis_amd.mask_head_stage(x, G, wt, b)
    got = devis_amd.mask_head_stage(x, G, wt, b, skip=torch.zeros(N, C, *HW, dtype=torch.float64, device=DEV))
    assert torch.equal(got, F.interpolate(plain, size=HW, mode="nearest"))
    from devis_amd import _mhstage
    for (a, A) in zip(hw, HW):
        want = F.interpolate(torch.arange(a, dtype=torch.float32, device=DEV).view(1, 1, a, 1), size=(A, 1)).flatten().long().tolist()
        assert [_mhstage.src_index(i, a, A) for i in range(A)] == want
    check_case(make_case(*case, torch.float64), torch.float64, what=str(case))


def test_tiling_boundaries():
    from devis_amd import _mhstage
    stat, tp, tc, bp = (_mhstage.tile(i) for i in range(4))
    h, w = 33, 37       # a group block of 4 channels exceeds one statistics tile; the pixels end inside every tile
    assert 4 * h * w > stat and (h * w) % tp and (h * w) % bp and h * w > 4 * bp
    check_case(make_case(2, 2, 8, 2, 3, (h, w), (h, w), torch.float32), torch.float32, what="two statistics tiles")
    check_case(make_case(2, 1, 8, 1, 0, (h, w), (41, 39), torch.bfloat16), torch.bfloat16, what="bf16, 3 statistics tiles")
    # C + E = 10 is no multiple of a 16-byte vector of any dtype, and no multiple of the channel tile
    assert 10 % tc
    for dtype in (torch.float32, torch.float16):
        check_case(make_case(2, 1, 9, 3, 1, (5, 7), (9, 14), dtype), dtype, what="C + E = 10 %s" % dtype)
    check_case(make_case(2, 2, 3 * tc + 8, 8, 5, (4, 5), (8, 9), torch.float32), torch.float32, what="a partial channel tile")


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("kind", ["repeat", "interleaved", "ragged", None, "permutation", "unused"])
def test_skip_index_patterns(kind, index_dtype):
    N, F_ = (6, 6) if kind in (None, "permutation") else (6, 3)
    d = make_case(N, F_, 16, 8, 4, (3, 5), (7, 9), torch.float32, kind=kind, index_dtype=index_dtype)
    _, grads = check_case(d, torch.float32, what="index %s %s" % (kind, index_dtype))
    if kind == "unused":
        assert float(grads["skip"][1].abs().max()) == 0.0 and float(grads["skip"][0].abs().max()) > 0


def test_grad_out_layouts_give_the_same_bits():
    d = make_case(6, 3, 24, 8, 8, (6, 10), (12, 20), torch.float32)
    go = grad_out_for(d, torch.float32).to(DEV)
    _, want = run_op(d, go)
    cl = go.contiguous(memory_format=torch.channels_last)
    big = torch.zeros(6, 40, 12, 24, device=DEV)
    big[:, 4:36, :, 2:22] = go
    view = big[:, 4:36, :, 2:22]
    assert not view.is_contiguous() and not view.is_contiguous(memory_format=torch.channels_last)
    for other in (cl, view):
        _, got = run_op(d, other)
        for name in want:
            assert torch.equal(got[name], want[name]), name


@pytest.mark.parametrize("need", [("x",), ("weight",), ("bias",), ("skip",), ("extra",), ("x", "skip"), ("weight", "bias"),
                                  ("x", "skip", "extra"), ("weight", "bias", "skip", "extra")])
def test_gradient_subsets_have_the_bits_of_the_full_backward(need):
    """("x", "skip", "extra") is a head with frozen GroupNorm parameters, the last subset one whose x is detached."""
    d = make_case(6, 3, 24, 8, 8, (6, 10), (12, 20), torch.float32)
    go = grad_out_for(d, torch.float32)
    _, full = run_op(d, go)
    _, got = run_op(d, go, need=need)
    assert sorted(got) == sorted(need)
    for name in need:
        assert torch.equal(got[name], full[name]), name


def test_extra_without_skip():
    d = make_case(4, 0, 16, 8, 8, (6, 10), (12, 20), torch.float32)
    assert d["skip"] is None
    check_case(d, torch.float32, what="extra alone")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_runs_give_identical_bits_also_in_deterministic_mode(dtype):
    d = make_case(6, 3, 64, 8, 8, (12, 20), (23, 40), dtype)
    go = grad_out_for(d, dtype)
    out, grads = run_op(d, go)
    for _ in range(2):
        out2, grads2 = run_op(d, go)
        assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            out2, grads2 = run_op(d, go)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_an_image_has_the_same_bits_alone_and_in_a_batch():
    d = make_case(6, 6, 24, 8, 4, (12, 20), (23, 40), torch.float32, kind=None)
    go = grad_out_for(d, torch.float32)
    out, grads = run_op(d, go)
    one = dict(d, x=d["x"][4:5], skip=d["skip"][4:5], extra=d["extra"][4:5])
    out1, grads1 = run_op(one, go[4:5])
    assert torch.equal(out1, out[4:5]) and torch.equal(grads1["x"], grads["x"][4:5])


# ---- degenerate values -----------------------------------------------------------------------------------------------

def test_constant_group_zero_channel_and_nan():
    import devis_amd
    d = make_case(3, 0, 16, 4, 0, (5, 7), (5, 7), torch.float32)
    x, wt, b = d["x"].clone(), d["weight"].clone(), d["bias"].clone()
    x[0, 4:8] = 2.5                         # a constant group: variance 0, z = bias exactly
    wt[13], b[13] = 0.0, 0.0                # z = 0: the gate is closed (strict >), the channel's dy exactly 0
    xd, wd, bd = x.to(DEV).requires_grad_(True), wt.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = devis_amd.mask_head_stage(xd, 4, wd, bd)
    gx, gw, gb = torch.autograd.grad(out, (xd, wd, bd), torch.ones_like(out))
    want = torch.relu(b[4:8]).view(4, 1, 1).expand(4, 5, 7)
    assert torch.equal(out[0, 4:8].cpu(), want)
    assert float(out[:, 13].abs().max()) == 0.0
    assert float(gw[13]) == 0.0 and float(gb[13]) == 0.0
    assert bool(gx.isfinite().all())
    x[1, 9, 2, 3] = float("nan")            # stays in group 2 of image 1
    out = devis_amd.mask_head_stage(x.to(DEV), 4, wt.to(DEV), bd.detach())
    bad = out.isnan()
    assert bool(bad[1, 8:12].all()) and int(bad.sum()) == 4 * 5 * 7


def test_no_images_and_no_extra_are_no_ops():
    import devis_amd
    x = torch.zeros(0, 16, 5, 7, device=DEV, requires_grad=True)
    wt, b = torch.ones(16, device=DEV, requires_grad=True), torch.zeros(16, device=DEV, requires_grad=True)
    skip = torch.zeros(2, 16, 9, 14, device=DEV, requires_grad=True)
    out = devis_amd.mask_head_stage(x, 8, wt, b, skip=skip, skip_index=torch.zeros(0, dtype=torch.int64, device=DEV))
    assert tuple(out.shape) == (0, 16, 9, 14)
    gx, gw, gb, gs = torch.autograd.grad(out, (x, wt, b, skip), torch.zeros_like(out))
    assert tuple(gx.shape) == (0, 16, 5, 7) and float(gw.abs().max()) == 0.0 and float(gs.abs().max()) == 0.0
    assert tuple(gs.shape) == (2, 16, 9, 14) and float(gb.abs().max()) == 0.0


# ---- output contract -------------------------------------------------------------------------------------------------

def test_the_convolution_reads_the_channels_last_result_without_a_copy():
    import devis_amd
    d = make_case(4, 2, 24, 8, 8, (6, 10), (12, 20), torch.float32)
    out, _ = run_op(d)
    assert out.is_contiguous(memory_format=torch.channels_last) and not out.is_contiguous()
    assert out.permute(0, 2, 3, 1).contiguous().data_ptr() == out.data_ptr()
    g = torch.Generator().manual_seed(5)
    weight = (0.1 * torch.randn(16, 32, 3, 3, generator=g)).to(DEV)
    offset, mask = (0.5 * torch.randn(4, 18, 12, 20, generator=g)).to(DEV), torch.rand(4, 9, 12, 20, generator=g).to(DEV)
    a = devis_amd.deform_conv2d(out, offset, weight, padding=(1, 1), mask=mask)
    b = devis_amd.deform_conv2d(out.contiguous(), offset, weight, padding=(1, 1), mask=mask)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_float32_out_parameters_and_maps_beside_16_bit_inputs(dtype):
    d = make_case(6, 3, 64, 8, 8, (6, 10), (12, 20), dtype)
    out, _ = check_case(d, dtype, out_dtype=torch.float32, what="%s, float32 out" % dtype)
    # the float32 result carries no storage rounding: it meets the f32 bar on the same 16-bit operands
    want = mhstage_oracle.mask_head_stage(d["x"], 8, d["weight"], d["bias"], 1e-5, d["skip"], d["index"], d["extra"])
    assert_close(out, want, TOL[torch.float32], "float32 out")
    d = make_case(6, 3, 64, 8, 8, (6, 10), (12, 20), dtype, param_dtype=torch.float32, extra_dtype=torch.float32)
    _, grads = check_case(d, dtype, what="%s, float32 parameters and maps" % dtype)
    assert grads["weight"].dtype == torch.float32 and grads["extra"].dtype == torch.float32 and grads["x"].dtype == dtype


# ---- module ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["maskhead_repeat", "maskhead_interleaved"])
def test_module_matches_the_reference_fixture_in_f64(name):
    from devis_amd.modules import MaskHeadConv
    d, state, features, bbox_mask = load_fixture(name)
    m = MaskHeadConv(64, [24], 8, False, [0, 1], 2).double()
    m.load_state_dict(state, strict=True)
    m = m.to(DEV)
    features = [f.to(DEV).requires_grad_(True) for f in features]
    bbox_mask = [b.to(DEV).requires_grad_(True) for b in bbox_mask]
    out = m(features, bbox_mask, 3, EXPANDS[name.split("_")[1]])
    params = dict(m.named_parameters())
    grads = torch.autograd.grad(out, features + bbox_mask + list(params.values()), d["grad_out"].to(DEV))
    assert_close(out.detach(), d["out"], 1e-10, name + " out")
    want = [d["grad/feature/%d" % i] for i in range(2)] + [d["grad/bbox_mask/%d" % i] for i in range(2)] + \
        [d["grad/state/" + n] for n in params]
    names = ["feature/0", "feature/1", "bbox_mask/0", "bbox_mask/1"] + list(params)
    for g, w_, nm in zip(grads, want, names):
        assert_close(g, w_, 1e-10, "%s grad %s" % (name, nm))


def eager_chain(m, features, bbox_mask, n, expand):
    """The reference's forward on the module's own layers and stock PyTorch glue."""
    x = torch.cat([expand(features[0], n), bbox_mask[0]], 1)
    x = F.relu(m.gn1(m.lay1(x)))
    x = F.relu(m.gn2(m.lay2(x)))
    for lvl, feature in enumerate(features[1:]):
        cur = expand(getattr(m, "adapter%d" % (lvl + 1))(feature), n)
        x = cur + F.interpolate(x, size=cur.shape[-2:], mode="nearest")
        if m.multi_scale_att_maps and lvl + 1 < len(bbox_mask):
            x = torch.cat([x, bbox_mask[lvl + 1]], 1)
        x = F.relu(getattr(m, "gn%d" % (lvl + 3))(getattr(m, "lay%d" % (lvl + 3))(x)))
    return m.out_lay(x)


def _head_and_inputs(seed=0):
    from devis_amd.modules import MaskHeadConv
    torch.manual_seed(seed)
    m = MaskHeadConv(64, [24, 16], 8, True, [0, 1, 2], 3)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.startswith("gn"):
                p.copy_(1 + 0.5 * torch.randn_like(p) if name.endswith("weight") else 0.3 * torch.randn_like(p))
            elif "offset_conv" in name or "modulator_conv" in name:
                p.copy_(0.05 * torch.randn_like(p))
    m = m.to(DEV)
    g = torch.Generator().manual_seed(seed + 1)
    sizes = [(5, 7), (9, 14), (18, 27)]
    features = [torch.randn(2, c, *s, generator=g).to(DEV).requires_grad_(True) for c, s in zip((64, 24, 16), sizes)]
    bbox_mask = [(0.5 * torch.randn(6, 8, *s, generator=g)).to(DEV).requires_grad_(True) for s in sizes]
    return m, features, bbox_mask


def test_f32_module_matches_the_pytorch_chain_with_hip_convolutions_on_both_sides():
    m, features, bbox_mask = _head_and_inputs()
    expand = EXPANDS["repeat"]
    leaves = features + bbox_mask + list(m.parameters())
    out = m(features, bbox_mask, 3, expand)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    got = torch.autograd.grad(out, leaves, go)
    want_out = eager_chain(m, features, bbox_mask, 3, expand)
    want = torch.autograd.grad(want_out, leaves, go)
    assert_close(out.detach(), want_out.detach().double().cpu(), 1e-4, "module out")
    for (name, _), g, w_ in zip([("feature%d" % i, 0) for i in range(3)] + [("map%d" % i, 0) for i in range(3)]
                                + list(m.named_parameters()), got, want):
        assert_close(g, w_.double().cpu(), 1e-4, "module grad " + name)


def test_autocast_module_matches_the_eager_autocast_chain():
    m, features, bbox_mask = _head_and_inputs(seed=2)
    expand = EXPANDS["repeat"]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = m(features, bbox_mask, 3, expand)
        want = eager_chain(m, features, bbox_mask, 3, expand)
    assert out.dtype == want.dtype
    assert_close(out.detach(), want.detach().double().cpu(), 1e-2, "autocast out")
    out.float().sum().backward()
    for name, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(p.grad.isfinite().all()), name


# ---- other execution modes -------------------------------------------------------------------------------------------

def test_compile_fullgraph_equals_eager_also_with_dynamic_shapes():
    import devis_amd
    fn = lambda x, w, b, s, i, e: devis_amd.mask_head_stage(x, 8, w, b, skip=s, skip_index=i, extra=e)      # noqa: E731
    compiled = torch.compile(fn, fullgraph=True)
    for N, hw, HW in ((6, (5, 7), (9, 14)), (9, (6, 10), (12, 20)), (3, (4, 6), (8, 11))):
        d = make_case(N, 3, 32, 8, 8, hw, HW, torch.float32)
        go = grad_out_for(d, torch.float32).to(DEV)
        want_out, want = run_op(d, go)
        t = {k: d[k].to(DEV).requires_grad_(True) for k in NAMES}
        idx = d["index"].to(DEV)
        for tensor, dims in ((t["x"], (0, 2, 3)), (t["skip"], (2, 3)), (t["extra"], (0, 2, 3)), (idx, (0,))):
            for dim in dims:
                torch._dynamo.mark_dynamic(tensor, dim)
        out = compiled(t["x"], t["weight"], t["bias"], t["skip"], idx, t["extra"])
        assert out.is_contiguous(memory_format=torch.channels_last)
        grads = torch.autograd.grad(out, [t[k] for k in NAMES], go)
        assert torch.equal(out, want_out)
        for k, g in zip(NAMES, grads):
            assert torch.equal(g, want[k]), k


def test_hip_graph_replay_with_changed_inputs_gives_the_changed_result():
    import devis_amd
    d = make_case(6, 3, 32, 8, 8, (6, 10), (12, 20), torch.float32)
    s = {k: d[k].to(DEV).clone() for k in NAMES}
    idx = d["index"].to(DEV)
    call = lambda t: devis_amd.mask_head_stage(t["x"], 8, t["weight"], t["bias"], skip=t["skip"], skip_index=idx,      # noqa: E731
                                               extra=t["extra"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(s)         # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(s)
    d2 = make_case(6, 3, 32, 8, 8, (6, 10), (12, 20), torch.float32, seed=5)
    for k in NAMES:
        s[k].copy_(d2[k])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, call({k: d2[k].to(DEV) for k in NAMES}))
    want = mhstage_oracle.mask_head_stage(d2["x"], 8, d2["weight"], d2["bias"], 1e-5, d2["skip"], d2["index"], d2["extra"])
    assert_close(out, want, 1e-4, "graph replay")
