"""GPU tests of the opt-in order-independent grad_input of the deformable convolution (devis_amd.reproducible_grad_input,
include/mdcn.h mdcn_backward_input_fixed): against the float64 oracle of tests/dcn_oracle.py with the tolerances of
tests/test_dcn_gpu.py (max|a - b| <= tol * max(1, max|b|), tol = 1e-4 f32, 1e-9 f64, 1e-2 bf16 / f16), bit for bit
against an integer restatement of the header's definition, and bit for bit against itself under everything the definition
says cannot show: run, chunking, batch, gradient subset, team size, the deterministic flag, compile and graph replay.

Inputs as in tests/test_dcn_gpu.py: offsets are multiples of 1/64 pixel that are never whole pixels.
"""
import math
from fractions import Fraction

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
    """The recipe of tests/test_dcn_gpu.py: CPU tensors already rounded to their storage types, and the geometry."""
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
    x, off, w, b, m, g = [None if t is None else (t.double() if dtype64 else t).to(device) for t in tensors]
    leaves = [x, off, m, w, b]
    for i, t in enumerate(leaves):
        if t is not None and (needs is None or needs[i]):
            t.requires_grad_(True)
    out = fn(x, off, w, b, mask=m, **geometry)
    wanted = [t for t in leaves if t is not None and t.requires_grad]
    got = iter(torch.autograd.grad(out, wanted, g))
    return [out.detach()] + [next(got) if t is not None and t.requires_grad else None for t in leaves]


def hip(tensors, geometry, needs=None, switch=True):
    """All six results with the switch as given around forward AND backward; the switch is restored."""
    import devis_amd
    with devis_amd.reproducible_grad_input(switch):
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


@pytest.fixture(autouse=True)
def _restore_flag_and_switch():
    import devis_amd
    flag, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    was = devis_amd.reproducible_grad_input_enabled()
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(flag, warn_only=warn)
        devis_amd.reproducible_grad_input(was)


# ---- 1. against the oracle -------------------------------------------------------------------------------------------

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


def test_the_cases_are_those_of_the_default_path():
    import test_dcn_gpu
    assert CASES == test_dcn_gpu.CASES and DTYPES == test_dcn_gpu.DTYPES and TOL == test_dcn_gpu.TOL


@pytest.mark.parametrize("dtype,off_dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("case", sorted(CASES))
def test_all_six_results_match_the_oracle_and_the_other_five_keep_their_bits(case, dtype, off_dtype):
    tensors, geometry = make_inputs(dtype=dtype, off_dtype=off_dtype, seed=len(case), **CASES[case])
    on, off = hip(tensors, geometry), hip(tensors, geometry, switch=False)
    assert on[1].dtype == dtype and on[1].shape == tensors[0].shape
    assert_close(on, oracle(tensors, geometry), TOL[dtype], case)
    for i in (0, 2, 3, 4, 5):
        assert (on[i] is None) == (off[i] is None)
        assert on[i] is None or torch.equal(on[i], off[i]), NAMES[i]


# ---- 2. bit for bit against an integer restatement -------------------------------------------------------------------

def _exponent(a_max, g_max, bound):
    """e of the quantum 2^e as include/mdcn.h defines it: A * G * bound <= 2^62 * 2^e from the exponents, then up to three
    halvings while the bound still holds."""
    ma, ea = math.frexp(a_max)
    mg, eg = math.frexp(g_max)
    en = (bound - 1).bit_length() if bound > 1 else 0
    e = ea + eg + en - 62
    r = ma * mg * (bound * 2.0 ** -en)
    for _ in range(3):
        if not 0 < r <= 0.5:
            break
        r, e = r * 2, e - 1
    return e


def _restated_grad_input(off, msk, gcol, N, C, H, W, G, K=3, pad=1):
    """grad_input [N, H, W, C] float32 of a 3x3 stride-1 convolution from the header's definition: f32 products in the stated
    order, each rounded to nearest-even onto the image's quantum with exact rational arithmetic, summed as Python integers,
    converted once."""
    Cg, P = C // G, H * W
    out = torch.empty(N, H, W, C, dtype=torch.float32)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)       # noqa: E731
    for n in range(N):
        a_max = float(msk[n].abs().max()) if msk is not None else 1.0
        g_max = float(gcol[n * P:(n + 1) * P].abs().max())
        e = _exponent(a_max, g_max, P * K * K)
        quantum = Fraction(2) ** e
        acc = [[[0] * C for _ in range(W)] for _ in range(H)]
        for ho in range(H):
            for wo in range(W):
                for k in range(K * K):
                    for g in range(G):
                        y = ho - pad + k // K + float(off[n, 2 * (g * K * K + k), ho, wo])
                        x = wo - pad + k % K + float(off[n, 2 * (g * K * K + k) + 1, ho, wo])
                        if not (-1 < y < H and -1 < x < W):
                            continue
                        y0, x0 = math.floor(y), math.floor(x)
                        ly, lx = f32(y - y0), f32(x - x0)
                        hy, hx = 1 - ly, 1 - lx
                        weights = (hy * hx, hy * lx, ly * hx, ly * lx)
                        # on the 1/64 grid the weights are exact products: nothing depends on how they are formed
                        exact = ((1 - (y - y0)) * (1 - (x - x0)), (1 - (y - y0)) * (x - x0), (y - y0) * (1 - (x - x0)), (y - y0) * (x - x0))
                        assert [float(v) for v in weights] == list(exact)
                        row = gcol[(n * H + ho) * W + wo, k * C + g * Cg:k * C + (g + 1) * Cg]
                        gm = row * msk[n, g * K * K + k, ho, wo] if msk is not None else row
                        for q, (yy, xx) in enumerate(((y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1))):
                            if not (0 <= yy < H and 0 <= xx < W):
                                continue
                            term = gm * weights[q]
                            assert term.dtype == torch.float32
                            cell = acc[yy][xx]
                            for c in range(Cg):
                                cell[g * Cg + c] += round(Fraction(float(term[c])) / quantum)      # ties to even
        ints = torch.tensor(acc, dtype=torch.int64)
        assert int(ints.abs().max()) < 2 ** 62
        out[n] = torch.ldexp(ints.to(torch.float32), torch.tensor(e))     # one rounding, then an exact scaling
    return out


@pytest.mark.parametrize("with_mask,G", [(True, 2), (False, 1)], ids=["mask_two_groups", "no_mask"])
def test_entry_point_equals_the_integer_restatement_bit_for_bit(with_mask, G):
    from devis_amd import _mdcn
    N, C, H, W, K = 2, 8, 5, 6, 3
    gen = torch.Generator().manual_seed(17 + G)
    whole = torch.randint(-2, 2, (N, 2 * G * K * K, H, W), generator=gen)
    off = ((whole * 64 + torch.randint(1, 64, whole.shape, generator=gen)).double() / 64).float()
    msk = (torch.rand(N, G * K * K, H, W, generator=gen) * 2) if with_mask else None
    # grad_columns over many binades, the second image far smaller than the first: its own quantum
    gcol = torch.randn(N * H * W, K * K * C, generator=gen) * torch.exp2(torch.randint(-12, 4, (N * H * W, 1), generator=gen).float())
    gcol[H * W:] *= 2.0 ** -9
    want = _restated_grad_input(off, msk, gcol, N, C, H, W, G)
    shape = _mdcn.Shape(N, C, H, W, H, W, K, K, 1, 1, 1, 1, 1, 1, G)
    ws = torch.empty(_mdcn.fixed_workspace_bytes(0, shape, N), dtype=torch.uint8, device=DEV).fill_(0xA5)     # need not be zero
    got = torch.full((N, H, W, C), float("nan"), device=DEV)
    _mdcn.backward_input_fixed(0, off.to(DEV), None if msk is None else msk.to(DEV), gcol.to(DEV), shape, ws, got)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()) and float(want.abs().max()) > 0
    assert torch.equal(got.cpu(), want)


# ---- 3. run to run ---------------------------------------------------------------------------------------------------

def test_two_runs_give_the_same_bits_in_all_six_results():
    tensors, geometry = make_inputs(N=4, C=72, Co=32, H=23, W=40, dtype=torch.float32, seed=31)
    a, b = hip(tensors, geometry), hip(tensors, geometry)
    for i in range(6):
        assert torch.equal(a[i], b[i]), NAMES[i]
    assert_close(a, oracle(tensors, geometry), 1e-4, "run to run")


# ---- 4. invariances --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [72, 64], ids=["c72_team32", "c64_team64"])
def test_grad_input_does_not_depend_on_chunking_batch_subset_or_flag(monkeypatch, C):
    from devis_amd.functions import deform_conv as D
    H, W = 9, 8
    tensors, geometry = make_inputs(N=4, C=C, Co=6, H=H, W=W, dtype=torch.float32, seed=C)
    whole = hip(tensors, geometry)[1]
    per_image = H * W * 9 * C * 4
    calls = []
    inner = D._mdcn.backward_input_fixed
    monkeypatch.setattr(D._mdcn, "backward_input_fixed", lambda code, off, *a: (calls.append(off.shape[0]), inner(code, off, *a))[1])
    for bound, want_calls in ((2 * per_image + per_image // 2, [2, 2]), (3 * per_image, [3, 1]), (1, [1, 1, 1, 1])):
        monkeypatch.setattr(D, "WORKSPACE_BYTES", bound)
        del calls[:]
        assert torch.equal(hip(tensors, geometry)[1], whole), "chunked under %d bytes" % bound
        assert calls == want_calls, calls
    monkeypatch.undo()
    x, off, w, b, m, g = tensors
    for n in range(4):
        alone = hip((x[n:n + 1], off[n:n + 1], w, b, m[n:n + 1], g[n:n + 1]), geometry)[1]
        assert torch.equal(alone[0], whole[n]), "image %d alone" % n
    only = hip(tensors, geometry, needs=[True, False, False, False, False])
    assert [t is not None for t in only[1:]] == [True, False, False, False, False]
    assert torch.equal(only[1], whole), "grad_input alone"
    torch.use_deterministic_algorithms(True)
    try:
        flagged = hip(tensors, geometry)[1]
    finally:
        torch.use_deterministic_algorithms(False)
    assert torch.equal(flagged, whole), "with torch.use_deterministic_algorithms(True)"


# ---- 5. non-finite ---------------------------------------------------------------------------------------------------

def test_an_infinite_mask_entry_marks_the_elements_its_tap_reaches_and_no_other():
    C, H, W = 8, 7, 9
    tensors, geometry = make_inputs(N=2, C=C, Co=4, H=H, W=W, dtype=torch.float32, seed=51, reach=1)
    x, off, w, b, m, g = tensors
    # a tap of image 1 whose four corners are all inside the map, and whose mask value is not the image's largest
    found = None
    for k in range(9):
        for ho in range(H):
            for wo in range(W):
                y, xx = ho - 1 + k // 3 + float(off[1, 2 * k, ho, wo]), wo - 1 + k % 3 + float(off[1, 2 * k + 1, ho, wo])
                if found is None and 0 < y < H - 1 and 0 < xx < W - 1 and float(m[1, k, ho, wo]) < float(m[1].max()):
                    found = (1, k, ho, wo)
    assert found is not None
    with_inf, with_zero = m.clone(), m.clone()
    with_inf[found], with_zero[found] = float("inf"), 0.0
    fixed = hip((x, off, w, b, with_inf, g), geometry)[1]
    default = hip((x, off, w, b, with_inf, g), geometry, switch=False)[1]
    base = hip((x, off, w, b, with_zero, g), geometry)[1]
    for kind in (torch.isnan, torch.isposinf, torch.isneginf):
        assert torch.equal(kind(fixed), kind(default)), kind.__name__
    reached = ~torch.isfinite(fixed)
    assert int(reached.sum()) == 4 * C and int(reached[0].sum()) == 0       # four corners, every channel, image 1 only
    assert bool(torch.isfinite(base).all())
    assert torch.equal(fixed[~reached], base[~reached])


# ---- 6. dynamic range ------------------------------------------------------------------------------------------------

def test_a_small_image_beside_a_large_one_keeps_its_own_precision():
    """The quantum is per image: an image whose grad_out is 2^-20 of its neighbour's meets the tolerance relative to ITS OWN
    largest gradient (no floor of 1 here: the floor would hide the small image altogether)."""
    tensors, geometry = make_inputs(N=2, C=16, Co=6, H=9, W=8, dtype=torch.float32, seed=61)
    x, off, w, b, m, g = tensors
    g = g.clone()
    g[1] *= 2.0 ** -20
    got = hip((x, off, w, b, m, g), geometry)[1].double().cpu()
    want = oracle((x, off, w, b, m, g), geometry)[1]
    for n in range(2):
        err, top = float((got[n] - want[n]).abs().max()), float(want[n].abs().max())
        print("image %d: err %.3e, largest %.3e" % (n, err, top))
        assert top > 0 and err <= 1e-4 * top, (n, err, top)
    assert float(want[1].abs().max()) < 2.0 ** -16 * float(want[0].abs().max())


# ---- 7. the module ---------------------------------------------------------------------------------------------------

def _modules(C, Co, bias, seed=0):
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


def _module_step(layer, x, g, autocast=None):
    xa = x.clone().requires_grad_(True)
    layer.zero_grad()
    if autocast is None:
        out = layer(xa)
    else:
        with torch.autocast("cuda", dtype=autocast):
            out = layer(xa)
    out.backward(g.to(out.dtype))
    torch.cuda.synchronize()
    return [out.detach(), xa.grad.clone()] + [p.grad.clone() for p in layer.parameters()]


def test_module_with_the_override_trains_under_the_deterministic_flag():
    ours, theirs = _modules(16, 8, bias=True)
    ours.reproducible_grad_input = True
    x = torch.randn(2, 16, 12, 20, generator=torch.Generator().manual_seed(1))
    g = torch.randn(2, 8, 12, 20, generator=torch.Generator().manual_seed(2))
    torch.use_deterministic_algorithms(True)
    try:
        a, b = _module_step(ours, x.to(DEV), g.to(DEV)), _module_step(ours, x.to(DEV), g.to(DEV))
        ours.reproducible_grad_input = None             # without the override (and the switch off) the layer refuses, as before
        with pytest.raises(RuntimeError, match="does not have a deterministic implementation"):
            _module_step(ours, x.to(DEV), g.to(DEV))
        ours.reproducible_grad_input = True
        c16, d16 = (_module_step(ours, x.to(DEV), g.to(DEV), torch.bfloat16) for _ in range(2))
    finally:
        torch.use_deterministic_algorithms(False)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for u, v in zip(c16, d16):
        assert torch.equal(u, v) and bool(torch.isfinite(u).all())
    assert c16[0].dtype == torch.bfloat16 and c16[1].dtype == torch.float32
    xb = x.double().requires_grad_(True)
    ref = theirs(xb)
    ref.backward(g.double())
    _close(a[0], ref, 1e-4, "out")
    _close(a[1], xb.grad, 1e-4, "x.grad")
    for got, (name, q) in zip(a[2:], theirs.named_parameters()):
        _close(got, q.grad, 1e-4, name)
    # under autocast, as tests/test_dcn_gpu.py compares it: the oracle on exactly the rounded operands the operator got
    # (bf16 input and weights, the float32 offsets and modulation the layer's own convolutions give under autocast)
    import devis_amd
    dt = torch.bfloat16
    xg = x.to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=dt):
        off = ours.offset_conv(xg).float()
        mod = 2. * torch.sigmoid(ours.modulator_conv(xg).float())
    w = ours.regular_conv.weight.detach().to(dt).double().cpu().requires_grad_(True)
    bias = ours.regular_conv.bias.detach().to(dt).double().cpu().requires_grad_(True)
    xr = x.to(dt).double().requires_grad_(True)
    ref16 = dcn_oracle.deform_conv2d(xr, off.double().cpu(), w, bias, 1, 1, 1, mod.double().cpu())
    ref16.backward(g.to(dt).double())
    names = [n for n, _ in ours.named_parameters()]
    _close(c16[0], ref16, 1e-2, "autocast out")
    _close(c16[2 + names.index("regular_conv.weight")], w.grad, 1e-2, "autocast regular_conv.weight.grad")
    _close(c16[2 + names.index("regular_conv.bias")], bias.grad, 1e-2, "autocast regular_conv.bias.grad")
    # grad_input of the operator on those operands, fixed-point, against the oracle's
    xo = x.to(DEV, dt).requires_grad_(True)
    out = devis_amd.deform_conv2d(xo, off, ours.regular_conv.weight.detach().to(dt), ours.regular_conv.bias.detach().to(dt),
                                  1, 1, 1, mod, reproducible_grad_input=True)
    gin, = torch.autograd.grad(out, [xo], g.to(DEV, dt))
    assert gin.dtype == dt
    _close(gin, xr.grad, 1e-2, "autocast operands grad_input")
    # and the layer's x.grad (which adds what flows back through its offset and modulator convolutions) against the
    # float-atomic layer's: the same terms summed the other way
    ours.reproducible_grad_input = False
    plain = _module_step(ours, x.to(DEV), g.to(DEV), dt)
    _close(c16[1], plain[1].double().cpu(), 1e-2, "autocast x.grad against the default path")


# ---- 8. compile and capture ------------------------------------------------------------------------------------------

def test_compiled_fullgraph_with_the_override_equals_eager():
    import devis_amd
    torch._dynamo.reset()
    try:
        # the operator with the call pinned, compiled: the same bits as eager in every result
        tensors, geometry = make_inputs(N=3, C=16, Co=6, H=9, W=8, G=2, seed=71)
        x, off, w, b, m, g = [t.to(DEV) for t in tensors]

        def op(x, off, w, b, m):
            return devis_amd.deform_conv2d(x, off, w, b, mask=m, reproducible_grad_input=True, **geometry)

        res = []
        torch.use_deterministic_algorithms(True)        # a pin that got lost on the way to the backward would raise here
        try:
            for fn in (op, torch.compile(op, fullgraph=True)):
                leaves = [t.clone().requires_grad_(True) for t in (x, off, w, b, m)]
                out = fn(*leaves)
                res.append([out.detach()] + list(torch.autograd.grad(out, leaves, g)))
            # the module with the override, compiled
            ours, _ = _modules(16, 8, bias=False, seed=6)
            ours.reproducible_grad_input = True
            xm = torch.randn(2, 16, 12, 20, generator=torch.Generator().manual_seed(7)).to(DEV)
            gm = torch.randn(2, 8, 12, 20, generator=torch.Generator().manual_seed(8)).to(DEV)
            eager = _module_step(ours, xm, gm)
            compiled = torch.compile(ours, fullgraph=True)
            xa = xm.clone().requires_grad_(True)
            ours.zero_grad()
            out = compiled(xa)
            out.backward(gm)
            traced = [out.detach(), xa.grad] + [p.grad.clone() for p in ours.parameters()]
        finally:
            torch.use_deterministic_algorithms(False)
        for u, v in zip(*res):
            assert torch.equal(u, v)
        for u, v in zip(eager, traced):
            assert float((u - v).abs().max()) <= 1e-4 * max(1.0, float(u.abs().max()))
    finally:
        torch._dynamo.reset()


def test_operator_with_the_switch_on_replays_from_a_hip_graph_with_changed_inputs():
    import devis_amd
    tensors, geometry = make_inputs(N=3, C=16, Co=6, H=9, W=8, G=2, seed=41)
    x, off, w, b, m, g = [t.to(DEV) for t in tensors]
    leaves = [t.requires_grad_(True) for t in (x, off, w, b, m)]

    def step():
        out = devis_amd.deform_conv2d(x, off, w, b, mask=m, **geometry)
        return (out,) + torch.autograd.grad(out, leaves, g)

    with devis_amd.reproducible_grad_input():
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
    graph.replay()                                      # (outside the with block: the graph holds the kernels it captured)
    torch.cuda.synchronize()
    got = [t.clone() for t in captured]
    # step() returns out, then the gradients of (x, off, w, b, m)
    assert_close([got[0], got[1], got[2], got[5], got[3], got[4]], oracle(fresh, geometry), 1e-4, "graph replay")
    assert torch.equal(got[1], hip(fresh, geometry)[1])             # and the bits of an eager run on the same inputs
