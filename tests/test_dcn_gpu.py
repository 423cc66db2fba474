"""GPU tests of the modulated deformable convolution (devis_amd.deform_conv2d, include/mdcn.h) against the float64 CPU
oracle of tests/dcn_oracle.py evaluated on the SAME ROUNDED inputs.  Error as everywhere in the project:
max|a - b| <= tol * max(1, max|b|) per tensor, tol = 1e-4 (f32), 1e-2 (bf16 / f16), 1e-9 (f64).

Random offsets are multiples of 1/64 pixel that are never whole pixels: exactly representable in every dtype and, added
to the integer base position, in float32 too -- the kernel and the oracle then agree on the cell of every point (bilinear
sampling has a kink at integer coordinates; the border tests put points exactly ON integers on purpose).
"""
import pytest
import torch

import dcn_oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = {torch.float32: 1e-4, torch.float64: 1e-9, torch.bfloat16: 1e-2, torch.float16: 1e-2}
NAMES = ("out", "grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _out_size(size, k, s, p, d):
    return (size + 2 * p - d * (k - 1) - 1) // s + 1


def make_inputs(N, C, Co, H, W, kernel=3, stride=1, padding=1, dilation=1, G=1, mask=True, bias=True, dtype=torch.float32,
                off_dtype=None, seed=0, reach=3):
    """CPU tensors already rounded to their storage types: (input, offset, weight, bias, mask, grad_out), and the geometry."""
    (Kh, Kw), (sh, sw), (ph, pw), (dh, dw) = _pair(kernel), _pair(stride), _pair(padding), _pair(dilation)
    Ho, Wo = _out_size(H, Kh, sh, ph, dh), _out_size(W, Kw, sw, pw, dw)
    gen = torch.Generator().manual_seed(seed)
    od = off_dtype or dtype
    x = torch.randn(N, C, H, W, generator=gen).to(dtype)
    whole = torch.randint(-reach, reach, (N, 2 * G * Kh * Kw, Ho, Wo), generator=gen)
    frac = torch.randint(1, 64, whole.shape, generator=gen)
    off = ((whole * 64 + frac).double() / 64).to(od)
    w = (torch.randn(Co, C, Kh, Kw, generator=gen) / (C * Kh * Kw) ** 0.5).to(dtype)
    b = torch.randn(Co, generator=gen).to(dtype) if bias else None
    m = (torch.rand(N, G * Kh * Kw, Ho, Wo, generator=gen) * 2).to(od) if mask else None
    g = torch.randn(N, Co, Ho, Wo, generator=gen).to(dtype)
    return (x, off, w, b, m, g), dict(stride=(sh, sw), padding=(ph, pw), dilation=(dh, dw))


def run(fn, tensors, geometry, device, dtype64=False, needs=None):
    """(out, grad_input, grad_offset, grad_mask, grad_weight, grad_bias) of `fn` on `device`; None where there is no tensor."""
    x, off, w, b, m, g = [None if t is None else (t.double() if dtype64 else t).to(device) for t in tensors]
    leaves = [x, off, m, w, b]
    for i, t in enumerate(leaves):
        if t is not None and (needs is None or needs[i]):
            t.requires_grad_(True)
    out = fn(x, off, w, b, mask=m, **geometry)
    wanted = [t for t in leaves if t is not None and t.requires_grad]
    got = iter(torch.autograd.grad(out, wanted, g))
    return [out.detach()] + [next(got) if t is not None and t.requires_grad else None for t in leaves]


def hip(tensors, geometry, needs=None):
    import devis_amd
    res = run(devis_amd.deform_conv2d, tensors, geometry, DEV, needs=needs)
    torch.cuda.synchronize()
    return res


def oracle(tensors, geometry):
    return run(dcn_oracle.deform_conv2d, tensors, geometry, "cpu", dtype64=True)


def assert_close(got, want, tol, what=""):
    for name, a, b in zip(NAMES, got, want):
        assert (a is None) == (b is None), (what, name)
        if a is None:
            continue
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        err = float((a.detach().double().cpu() - b).abs().max())
        bound = tol * max(1.0, float(b.abs().max()))
        print("%s %s: err %.3e bound %.3e" % (what, name, err, bound))
        assert err <= bound, (what, name, err, bound)


# ---- the operator against the oracle ---------------------------------------------------------------------------------

CASES = {
    "3x3_g1_mask_bias": dict(N=3, C=8, Co=5, H=9, W=11),
    "3x2_g2_strided_dilated_nomask": dict(N=2, C=8, Co=4, H=10, W=13, kernel=(3, 2), stride=(2, 1), padding=(2, 0),
                                          dilation=(1, 2), G=2, mask=False),
    "1x1_g4_stride2_nobias": dict(N=2, C=16, Co=3, H=9, W=12, kernel=1, stride=2, padding=0, G=4, bias=False),
    "3x3_g2_dil2_pad2_c6": dict(N=2, C=6, Co=7, H=8, W=7, dilation=2, padding=2, G=2),
    "3x3_c72_co1_nomask_nobias": dict(N=2, C=72, Co=1, H=7, W=10, mask=False, bias=False),
    "3x3_c136_g1": dict(N=1, C=136, Co=9, H=6, W=5),
}
DTYPES = [(torch.float32, None), (torch.float64, None), (torch.bfloat16, None), (torch.float16, None),
          (torch.bfloat16, torch.float32), (torch.float16, torch.float32)]


@pytest.mark.parametrize("dtype,off_dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("case", sorted(CASES))
def test_forward_and_all_gradients_match_the_oracle(case, dtype, off_dtype):
    tensors, geometry = make_inputs(dtype=dtype, off_dtype=off_dtype, seed=len(case), **CASES[case])
    got = hip(tensors, geometry)
    assert got[0].dtype == dtype and got[2].dtype == (off_dtype or dtype)
    assert_close(got, oracle(tensors, geometry), TOL[dtype], case)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_chunked_under_a_small_workspace_bound_gives_the_same_result(monkeypatch, dtype):
    """N = 7 in chunks of 2 images (4 chunks, the last one short): `out` bit for bit what one chunk gives."""
    from devis_amd.functions import deform_conv as D
    tensors, geometry = make_inputs(N=7, C=16, Co=6, H=9, W=8, G=2, dtype=dtype, seed=5)
    whole = hip(tensors, geometry)
    per_image = 9 * 8 * 9 * 16 * tensors[0].element_size()
    chunks = []
    inner = D._mdcn.im2col
    monkeypatch.setattr(D._mdcn, "im2col", lambda code, x, *a: (chunks.append(x.shape[0]), inner(code, x, *a))[1])
    monkeypatch.setattr(D, "WORKSPACE_BYTES", 2 * per_image + per_image // 2)
    cut = hip(tensors, geometry)
    assert chunks == [2, 2, 2, 1] * 2, chunks           # forward, then the backward's columns for grad_weight
    assert torch.equal(cut[0], whole[0])
    assert_close(cut, oracle(tensors, geometry), TOL[dtype], "chunked")
    monkeypatch.setattr(D, "WORKSPACE_BYTES", 1)        # below one image: one image per chunk
    del chunks[:]
    assert torch.equal(hip(tensors, geometry)[0], whole[0]) and chunks == [1] * 14


# ---- borders ---------------------------------------------------------------------------------------------------------

def _border_inputs(dtype):
    """One 1x1 tap per output pixel of a 6x7 map, its offset chosen per pixel: rows put the point in (-1, 0), on integers,
    on H-1, in (H-1, H), at H exactly, outside by a pixel and by 1e9, and on NaN, +inf and -inf: in the row, in the column and
    in both (a pixel's row entry i meets column entries i, i + 1 and i + 2)."""
    H, W = 6, 7
    tensors, geometry = make_inputs(N=1, C=8, Co=3, H=H, W=W, kernel=1, padding=0, dtype=dtype, seed=3)
    x, off, w, b, m, g = tensors
    nan, inf = float("nan"), float("inf")
    ys = torch.tensor([-0.5, 0.0, 2.0, H - 1.0, H - 0.25, -1.5, float(H), 1e9, -1e9, 2.5, nan, inf, -inf, 1.5])
    xs = torch.tensor([-0.75, 0.0, 3.0, W - 1.0, W - 0.5, -2.0, float(W), 3e9, -3e9, 1.25, 2.5, nan, inf, -inf])
    off = off.double()
    for ho in range(H):
        for wo in range(W):
            i = (ho * W + wo) % len(ys)
            j = (ho * W + wo) // len(ys) + i
            off[0, 0, ho, wo] = ys[i] - ho
            off[0, 1, ho, wo] = xs[j % len(xs)] - wo
    return (x, off.to(tensors[1].dtype), w, b, m, g), geometry


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16, torch.float16], ids=["f32", "f64", "bf16", "f16"])
def test_points_on_and_beyond_the_border(dtype):
    tensors, geometry = _border_inputs(dtype)
    got, want = hip(tensors, geometry), oracle(tensors, geometry)
    assert all(bool(torch.isfinite(t).all()) for t in got + want if t is not None)
    assert_close(got, want, TOL[dtype], "border")
    # a point at or beyond one pixel outside contributes nothing and has zero gradients, exactly
    x, off = tensors[0], tensors[1].double()
    H, W = x.shape[2:]
    ho, wo = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    y, xx = off[0, 0] + ho, off[0, 1] + wo
    outside = ~((y > -1) & (y < H) & (xx > -1) & (xx < W))                      # (with NaN: outside)
    assert int(outside.sum()) >= 8 and int((y.isnan() | xx.isnan()).sum()) >= 5 and int((y.isinf() | xx.isinf()).sum()) >= 8
    bias = tensors[3].to(DEV).view(-1, 1)
    assert torch.equal(got[0][0][:, outside.to(DEV)], bias.expand(-1, int(outside.sum())))
    assert float(got[2][0][:, outside.to(DEV)].abs().max()) == 0 and float(got[3][0][:, outside.to(DEV)].abs().max()) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_a_non_finite_tap_of_a_3x3_kernel_stays_in_its_own_tap(dtype):
    """NaN, +inf and -inf row and column offsets in single taps of a 3x3 kernel over two groups of two channels, and in every tap
    of one pixel: the tap contributes nothing and its grad_offset / grad_mask are exactly 0, and neither the wavefront reduction nor
    the team padding of mdcn_backward_kernel carries it anywhere -- every output is finite, matches the oracle, and keeps its bits
    when those taps point far outside the map instead (grad_input: float atomics, to rounding)."""
    tensors, geometry = make_inputs(N=2, C=4, Co=5, H=6, W=7, G=2, dtype=dtype, seed=13)
    x, off, w, b, m, g = tensors
    off, far = off.clone(), off.clone()
    bad = torch.zeros_like(m, dtype=torch.bool)                                 # [N, G*K, Ho, Wo]
    vals = [float("nan"), float("inf"), float("-inf")]
    taps = [(t % 2, t, t % 6, (2 * t + 1) % 7) for t in range(18)] + [(0, k, 3, 3) for k in range(9)]
    for i, (n, t, ho, wo) in enumerate(taps):
        where = (i // 3) % 3                                                    # 0: row, 1: column, 2: both
        bad[n, t, ho, wo] = True
        for axis in ((0,), (1,), (0, 1))[where]:
            off[n, 2 * t + axis, ho, wo] = vals[i % 3]
        far[n, 2 * t, ho, wo] = far[n, 2 * t + 1, ho, wo] = -100.0
    got, want = hip((x, off, w, b, m, g), geometry), oracle((x, off, w, b, m, g), geometry)
    assert all(bool(torch.isfinite(t).all()) for t in got + want)
    assert_close(got, want, TOL[dtype], "non-finite taps")
    sel = bad.to(DEV)
    assert float(got[3][sel].abs().max()) == 0                                  # grad_mask, grad_offset of both axes
    assert float(got[2].view(2, 18, 2, 6, 7)[:, :, 0][sel].abs().max()) == 0 and float(got[2].view(2, 18, 2, 6, 7)[:, :, 1][sel].abs().max()) == 0
    moved = hip((x, far, w, b, m, g), geometry)
    for i in (0, 2, 3, 4, 5):
        assert torch.equal(got[i], moved[i]), NAMES[i]
    assert float((got[1] - moved[1]).abs().max()) <= TOL[dtype] * max(1.0, float(moved[1].abs().max()))


def test_scatter_writes_nothing_outside_grad_input():
    """mdcn_backward on an accumulator with guard rows before and after it: every point of the border case, plus taps of a
    3x3 kernel with wild offsets; the guards keep their pattern and the inside equals the oracle's grad_input."""
    from devis_amd import _mdcn
    tensors, geometry = make_inputs(N=2, C=8, Co=4, H=6, W=7, G=2, dtype=torch.float32, seed=9, reach=9)
    x, off, w, b, m, g = tensors
    off[:, :, 0, :] = torch.tensor([-1e9, -7.0, -1.0, -0.5, 6.5, 7.0, 1e9])     # a row of extremes on top of the wild ones
    want = oracle((x, off, w, b, m, g), geometry)[1]
    N, C, H, W = x.shape
    K, G, P = 9, 2, H * W
    shape = _mdcn.Shape(N, C, H, W, H, W, 3, 3, 1, 1, 1, 1, 1, 1, G)
    x_cl = x.to(DEV).permute(0, 2, 3, 1).contiguous()
    gcol = (g.to(DEV).permute(0, 2, 3, 1).reshape(N * P, -1) @ w.to(DEV).permute(0, 2, 3, 1).reshape(w.shape[0], K * C)).contiguous()
    guard = 4 * W * C
    buf = torch.full((guard + N * H * W * C + guard,), 12345.0, device=DEV)
    acc = buf[guard:guard + N * H * W * C].view(N, H, W, C)
    acc.zero_()
    goff, gmsk = torch.empty_like(off, device=DEV), torch.empty_like(m, device=DEV)
    _mdcn.backward(_mdcn.GRAD_INPUT | _mdcn.GRAD_SAMPLING, 0, x_cl, off.to(DEV), m.to(DEV), gcol, shape, acc, goff, gmsk)
    torch.cuda.synchronize()
    assert bool((buf[:guard] == 12345.0).all()) and bool((buf[-guard:] == 12345.0).all())
    got = acc.permute(0, 3, 1, 2).double().cpu()
    assert float((got - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))


# ---- the reference mask head's six layers ----------------------------------------------------------------------------

MASK_HEAD = [(264, 264, 12, 20), (264, 128, 12, 20), (136, 64, 23, 40), (72, 32, 45, 80), (32, 16, 90, 160), (16, 1, 90, 160)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layer", MASK_HEAD, ids=lambda l: "c%d_co%d_%dx%d" % l)
def test_mask_head_layers_of_a_360x640_clip(layer, dtype):
    C, Co, H, W = layer
    tensors, geometry = make_inputs(N=12, C=C, Co=Co, H=H, W=W, dtype=dtype, seed=C + Co, reach=2)
    assert_close(hip(tensors, geometry), oracle(tensors, geometry), TOL[dtype], "layer %s" % (layer,))


# ---- gradcheck -------------------------------------------------------------------------------------------------------

def test_gradcheck_of_the_f64_hip_path():
    import devis_amd
    gen = torch.Generator().manual_seed(11)
    N, C, Co, H, W, G, K = 2, 4, 3, 5, 6, 2, 9
    whole = torch.randint(-2, 3, (N, 2 * G * K, H, W), generator=gen).double()
    frac = 0.1 + 0.8 * torch.rand(whole.shape, generator=gen, dtype=torch.float64)      # built, not filtered
    off = whole + frac
    # every sample coordinate = integer base + offset: its fractional part is the offset's
    assert bool(((off - off.floor() >= 0.1) & (off - off.floor() <= 0.9)).all())
    x = torch.randn(N, C, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(Co, C, 3, 3, generator=gen, dtype=torch.float64)
    b = torch.randn(Co, generator=gen, dtype=torch.float64)
    m = torch.rand(N, G * K, H, W, generator=gen, dtype=torch.float64)
    leaves = [t.to(DEV).requires_grad_(True) for t in (x, off, w, b, m)]
    assert torch.autograd.gradcheck(lambda x, o, w, b, m: devis_amd.deform_conv2d(x, o, w, b, 1, 1, 1, m), leaves,
                                    nondet_tol=1e-10)


# ---- gradient subsets, run to run ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_each_gradient_alone_equals_the_full_backward(dtype):
    tensors, geometry = make_inputs(N=3, C=16, Co=6, H=9, W=8, G=2, dtype=dtype, seed=21)
    full = hip(tensors, geometry)
    for i, name in enumerate(NAMES[1:]):
        alone = hip(tensors, geometry, needs=[j == i for j in range(5)])
        assert [t is not None for t in alone[1:]] == [j == i for j in range(5)]
        if name == "grad_input":        # float atomics: the order of the adds differs
            err = float((alone[1].double() - full[1].double()).abs().max())
            assert err <= TOL[dtype] * max(1.0, float(full[1].double().abs().max())), err
        else:
            assert torch.equal(alone[1 + i], full[1 + i]), name


def test_two_launches_give_the_same_bits_except_grad_input():
    tensors, geometry = make_inputs(N=4, C=72, Co=32, H=23, W=40, dtype=torch.float32, seed=31)
    a, b = hip(tensors, geometry), hip(tensors, geometry)
    for i in (0, 2, 3, 4, 5):
        assert torch.equal(a[i], b[i]), NAMES[i]
    assert float((a[1] - b[1]).abs().max()) <= 1e-4 * max(1.0, float(a[1].abs().max()))


def test_deterministic_mode_on_the_gpu():
    tensors, geometry = make_inputs(N=1, C=8, Co=2, H=5, W=5, seed=2)
    try:
        torch.use_deterministic_algorithms(True)
        with pytest.raises(RuntimeError, match="deform_conv2d_backward does not have a deterministic implementation"):
            hip(tensors, geometry)
        got = hip(tensors, geometry, needs=[False, True, True, True, True])
        torch.use_deterministic_algorithms(False)
        assert all(torch.equal(a, b) for a, b in zip(got[2:], hip(tensors, geometry)[2:]))
    finally:
        torch.use_deterministic_algorithms(False)


# ---- the module ------------------------------------------------------------------------------------------------------

def _modules(C, Co, bias, seed=0):
    """The HIP module on the GPU and the oracle module in float64 on the CPU with the same, non-trivial parameters."""
    from devis_amd.modules import ModulatedDeformableConv2d
    torch.manual_seed(seed)
    ours = ModulatedDeformableConv2d(C, Co, bias=bias)
    with torch.no_grad():
        for conv, scale in ((ours.offset_conv, 0.3), (ours.modulator_conv, 0.3)):
            conv.weight.normal_(0, scale / (C * 9) ** 0.5 * 3)
            conv.bias.normal_(0, scale)
    theirs = dcn_oracle.ModulatedDeformableConv2d(C, Co, bias=bias).double()
    theirs.load_state_dict({k: v.double() for k, v in ours.state_dict().items()}, strict=True)
    return ours.to(DEV), theirs


def _close(a, b, tol, what):
    err = float((a.detach().double().cpu() - b.detach()).abs().max())
    bound = tol * max(1.0, float(b.detach().abs().max()))
    print("%s: err %.3e bound %.3e" % (what, err, bound))
    assert err <= bound, (what, err, bound)


def test_module_forward_and_backward_match_the_oracle_module():
    ours, theirs = _modules(16, 8, bias=True)
    x = torch.randn(2, 16, 12, 20, generator=torch.Generator().manual_seed(1))
    g = torch.randn(2, 8, 12, 20, generator=torch.Generator().manual_seed(2))
    xa, xb = x.to(DEV).requires_grad_(True), x.double().requires_grad_(True)
    out, ref = ours(xa), theirs(xb)
    out.backward(g.to(DEV))
    ref.backward(g.double())
    _close(out, ref, 1e-4, "out")
    _close(xa.grad, xb.grad, 1e-4, "x.grad")
    for (name, p), (_, q) in zip(ours.named_parameters(), theirs.named_parameters()):
        _close(p.grad, q.grad, 1e-4, name)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_module_under_autocast(dtype):
    """Under autocast the operator gets a 16-bit input and weights and float32 offsets / modulation; it is compared with the
    oracle on exactly those rounded operands (the offsets as the module's own convolutions give them under autocast)."""
    ours, _ = _modules(16, 8, bias=True, seed=3)
    x = torch.randn(2, 16, 12, 20, generator=torch.Generator().manual_seed(4)).to(DEV).requires_grad_(True)
    g = torch.randn(2, 8, 12, 20, generator=torch.Generator().manual_seed(5)).to(dtype)
    with torch.autocast("cuda", dtype=dtype):
        out = ours(x)
        off = ours.offset_conv(x).float().detach()
        mod = (2. * torch.sigmoid(ours.modulator_conv(x).float())).detach()
    assert out.dtype == dtype and off.dtype == torch.float32
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    assert x.grad is not None and x.grad.dtype == torch.float32 and bool(torch.isfinite(x.grad).all())
    w = ours.regular_conv.weight.detach().to(dtype).double().cpu().requires_grad_(True)
    b = ours.regular_conv.bias.detach().to(dtype).double().cpu().requires_grad_(True)
    ref = dcn_oracle.deform_conv2d(x.detach().to(dtype).double().cpu(), off.double().cpu(), w, b, 1, 1, 1, mod.double().cpu())
    ref.backward(g.double())
    _close(out, ref, 1e-2, "out")
    _close(ours.regular_conv.weight.grad, w.grad, 1e-2, "regular_conv.weight.grad")
    _close(ours.regular_conv.bias.grad, b.grad, 1e-2, "regular_conv.bias.grad")
    assert ours.offset_conv.weight.grad is not None and ours.modulator_conv.weight.grad is not None


def test_module_compiles_fullgraph_and_matches_eager():
    torch._dynamo.reset()
    ours, _ = _modules(16, 8, bias=False, seed=6)
    compiled = torch.compile(ours, fullgraph=True)
    x = torch.randn(2, 16, 12, 20, generator=torch.Generator().manual_seed(7)).to(DEV)
    g = torch.randn(2, 8, 12, 20, generator=torch.Generator().manual_seed(8)).to(DEV)
    res = []
    for fn in (ours, compiled):
        xa = x.clone().requires_grad_(True)
        ours.zero_grad()
        out = fn(xa)
        out.backward(g)
        res.append([out.detach(), xa.grad] + [p.grad.clone() for p in ours.parameters()])
    for a, b in zip(*res):
        assert float((a - b).abs().max()) <= 1e-4 * max(1.0, float(a.abs().max()))
    torch._dynamo.reset()


def test_operator_replays_from_a_hip_graph_with_changed_inputs():
    import devis_amd
    tensors, geometry = make_inputs(N=3, C=16, Co=6, H=9, W=8, G=2, seed=41)
    x, off, w, b, m, g = [t.to(DEV) for t in tensors]
    leaves = [t.requires_grad_(True) for t in (x, off, w, b, m)]

    def step():
        out = devis_amd.deform_conv2d(x, off, w, b, mask=m, **geometry)
        return (out,) + torch.autograd.grad(out, leaves, g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    fresh, _ = make_inputs(N=3, C=16, Co=6, H=9, W=8, G=2, seed=42)
    with torch.no_grad():
        for t, new in zip((x, off, w, b, m, g), fresh):
            t.copy_(new.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in captured]
    want = oracle(fresh, geometry)
    # step() returns out, then the gradients of (x, off, w, b, m)
    assert_close([got[0], got[1], got[2], got[5], got[3], got[4]], want, 1e-4, "graph replay")
