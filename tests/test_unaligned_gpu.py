"""GPU: every kernel route on contiguous operands that are not 16-byte aligned -- views at an odd offset of a flat buffer, as
`x[1:]`, a piece of torch.split with an odd row size or a parameter inside a flattened bucket are.  The dispatcher decides
from the pointers at every call whether a kernel may use 16-byte accesses (csrc/msda_plan.hip: fast_path_takes for value, out,
grad_out and grad_value; wide_loads / wide_stores for the sampling arrays and their gradients), and tensors fresh from the
caching allocator only ever select the wide side of those decisions.

Every shifted tensor sits inside a buffer filled with a NaN bit pattern: `shifted` asserts that its pointer is off by the
bytes asked for -- which is what selects the narrow code, alignment being a function of the pointer alone -- and, after the
call, `canaries_intact` that nothing round it was written.  Outputs start as NaN, so an element the narrow stores skip is not
finite.  Inputs, oracles, tolerances and the route labels are those of tests/test_layout_gpu.py; the last test asserts that
every label of LABELS was reached by a passing case."""
import functools

import numpy as np
import pytest
import torch

from helpers import PYR_A, relayout
from test_layout_gpu import (DEC_ROUTES, DTYPES, MFMA_SHAPES, OP_CASES, ROUTES, SMALL, _decoder_call, _env, _mark, _np, _pin,
                             _rounded, _t, check, op_case, op_reference, run_op, run_temporal, temporal_case,
                             temporal_reference_clips)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEEN = set()
# the labels of test_layout_gpu.ROUTES the cases below reach on shifted operands
LABELS = ("fwd tile", "fwd tile, several waves", "fwd resident-slab nt1", "fwd resident-slab nt2", "fwd resident-slab nt4",
          "fwd resident-window", "fwd generic", "gather tile", "gather resident-slab", "gather resident-slab, frame split",
          "gather resident-window", "bwd generic", "scatter owner, level order", "scatter owner, image order",
          "scatter LDS atomics", "bwd global atomics", "scatter matrix-pipe NL=1", "scatter matrix-pipe NL=2",
          "scatter owner, grad_value in the storage type", "scatter matrix-pipe, grad_value in the storage type",
          "value only (culling records)", "sampling only")
assert set(LABELS) <= set(ROUTES)


# ---- placement ------------------------------------------------------------------------------------------------------------------
# shifts in elements: with the element sizes they give the 2-, 4-, 8- and 12-byte residues
SHIFTS = {torch.float32: (1, 2, 3), torch.bfloat16: (1, 2, 4), torch.float16: (1, 2, 4), torch.float64: (1, 1, 1), torch.bool: (1, 2, 3)}
# canary bit patterns (NaNs of the floating types), written and compared through an integer view
_CANARY = {torch.float32: (torch.int32, 0x7fc12345), torch.float64: (torch.int64, 0x7ff8000000012345),
           torch.bfloat16: (torch.int16, 0x7fc1), torch.float16: (torch.int16, 0x7e01), torch.bool: (torch.uint8, 1)}


def _bits(buf):
    return buf.view(_CANARY[buf.dtype][0])


def shifted(t, k):
    """`t` copied into a contiguous view that starts k elements off a 16-byte boundary, inside a buffer of canaries;
    returns (view, buffer)."""
    n = t.numel()
    buf = torch.empty(n + 32, dtype=t.dtype, device=DEV)
    _bits(buf).fill_(_CANARY[t.dtype][1])
    view = buf[16 + k:16 + k + n].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.contiguous().data_ptr() == view.data_ptr()
    assert view.data_ptr() % 16 == (k * t.element_size()) % 16 != 0, (view.data_ptr() % 16, k, t.dtype)
    return view, buf


def canaries_intact(buf, k, numel, what=""):
    """The 16 + k elements before and the 16 - k elements after the view of `shifted` still hold the canary bits."""
    bits, want = _bits(buf), _CANARY[buf.dtype][1]
    before, after = bits[:16 + k], bits[16 + k + numel:]
    assert before.numel() == 16 + k and after.numel() == 16 - k
    assert bool((before == want).all()), ("written before the tensor", what)
    assert bool((after == want).all()), ("written past the tensor", what)


LOC_NAMES = ("loc", "aw", "loc_c", "aw_c", "loc_t", "aw_t")


class Place:
    """The `place` argument of run_op / run_temporal: operand or output `name` goes k = shifts[name] elements off alignment.
    `loc32`: the sampling tensors are float32 (beside a 16-bit value: the *_LOC32 type codes)."""

    def __init__(self, shifts, loc32=False):
        self.shifts, self.loc32, self.held, self.tensors = {n: k for n, k in shifts.items() if k}, loc32, {}, {}

    def __call__(self, name, t):
        if self.loc32 and name in LOC_NAMES:
            t = t.float()
        if name in self.shifts:
            t, buf = shifted(t, self.shifts[name])
            self.held[name] = (buf, self.shifts[name], t.numel())
        self.tensors[name] = t
        return t

    def check(self):
        assert set(self.held) == set(self.shifts), (sorted(self.held), sorted(self.shifts))
        for name, (buf, k, n) in self.held.items():
            canaries_intact(buf, k, n, name)


SAME_ROUTE = ("points", "last-of-four", "gradients", "points+gradients")


def shifts_of(case, dtype, temporal, loc_dtype=None):
    """The operands case `case` of the module shifts, and by how many elements (fp32 points: loc +1, aw +2, loc_t +3, aw_t +1)."""
    a, b, c = SHIFTS[loc_dtype or dtype]
    va, vb, vc = SHIFTS[dtype]
    pts = ("loc_c", "aw_c", "loc_t", "aw_t") if temporal else ("loc", "aw")
    points = dict(zip(pts, (a, b, c, a)))
    grads = {"grad_" + n: k for n, k in zip(pts, (b, c, a, b))}
    arith = SHIFTS[torch.float64 if dtype == torch.float64 else torch.float32]
    table = {"points": points, "last-of-four": {pts[-1]: c}, "gradients": grads, "points+gradients": dict(points, **grads),
             "value": {"value": va}, "out": {"out": vb}, "grad_out": {"grad_out": vc}, "grad_value": {"grad_value": arith[2]}}
    table["everything"] = dict(table["points+gradients"], value=va, out=vb, grad_out=vc, grad_value=arith[2])
    return table[case]


def routes_as_expected(case, routes, aligned):
    """Shifted sampling tensors and sampling gradients keep the aligned call's kernels; a shifted value, out, grad_out or
    grad_value sends its direction to the generic kernels, whatever family the environment forces."""
    fwd_generic = case in ("value", "out", "everything")
    bwd_generic = case in ("value", "grad_out", "grad_value", "everything")
    if fwd_generic:
        _mark("fwd generic", routes[0], seen=SEEN)
    else:
        assert routes[0] == aligned[0], (routes[0], aligned[0])
    if bwd_generic:
        _mark("bwd generic", routes[1], seen=SEEN)
    else:
        assert routes[1] == aligned[1], (routes[1], aligned[1])


_ALIGNED = {}


def aligned_routes(key, run):
    """(forward, backward) routes of the call with every operand aligned, made once per `key`."""
    if key not in _ALIGNED:
        _ALIGNED[key] = run()[1]
    return _ALIGNED[key]


# ---- the decoder call of DeVIS on every route of DEC_ROUTES --------------------------------------------------------------------
def decoder_case(case, env, pins, monkeypatch, dtype=torch.float32, size=(), grads=3, loc32=False, key=None):
    from devis_amd import _native
    _env(monkeypatch, env)
    r, ref = _decoder_call("tail_gap", dtype, *size)
    pinned = _pin(r, pins) if pins else None
    place = Place(shifts_of(case, dtype, True, torch.float32 if loc32 else None), loc32)
    try:
        got, routes = run_temporal(r, dtype, grads=grads, place=place)
        aligned = aligned_routes((key, dtype, grads, loc32), lambda: run_temporal(r, dtype, grads=grads, place=Place({}, loc32)))
    finally:
        if pinned:
            _native.pin_route(pinned, "")
    place.check()
    check(got, ref, r, dtype)
    routes_as_expected(case, routes, aligned)
    return routes, place


@pytest.mark.parametrize("case", SAME_ROUTE)
@pytest.mark.parametrize("fwd,bwd,env,pins", DEC_ROUTES, ids=[a for a, *_ in DEC_ROUTES])
def test_decoder_call_routes_on_shifted_sampling_tensors(fwd, bwd, env, pins, case, monkeypatch):
    (rf, rb), _ = decoder_case(case, env, pins, monkeypatch, key=fwd)
    _mark(fwd, rf, seen=SEEN)
    for b in bwd:
        _mark(b, rb, seen=SEEN)


@pytest.mark.parametrize("case", ["value", "out", "grad_out", "grad_value"])
def test_decoder_call_with_a_shifted_value_output_or_gradient_takes_the_generic_kernels(case, monkeypatch):
    """The environment forces the resident-slab family; the pointer rule of fast_path_takes overrides it."""
    fwd, bwd, env, pins = DEC_ROUTES[0]
    decoder_case(case, env, pins, monkeypatch, key=fwd)


@pytest.mark.parametrize("grads,case,label", [(1, "points", "value only (culling records)"), (2, "gradients", "sampling only")],
                         ids=["value", "sampling"])
def test_decoder_call_gradient_subsets(grads, case, label, monkeypatch):
    fwd, bwd, env, pins = DEC_ROUTES[0]
    (rf, rb), place = decoder_case(case, env, pins, monkeypatch, grads=grads, key=fwd)
    assert ("grad_value" in place.tensors) == (grads == 1) and ("grad_loc_c" in place.tensors) == (grads == 2)
    _mark(label, rb, seen=SEEN)


# ---- 16-bit storage: grad_value in the storage type needs value, grad_out and grad_value aligned ------------------------------
SMALL_DECODER = (4, 100)            # T, Lq of test_decoder_call_grad_value_in_the_storage_type


def _storage_label(mfma):
    return "scatter matrix-pipe, grad_value in the storage type" if mfma == "1" else "scatter owner, grad_value in the storage type"


@pytest.mark.parametrize("case", ["points", "gradients"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("mfma", ["0", "1"])
def test_16bit_decoder_call_keeps_grad_value_in_the_storage_type(mfma, dtype, case, monkeypatch):
    dt = DTYPES[dtype]
    (rf, rb), place = decoder_case(case, {"MSDA_SCATTER_MFMA": mfma}, None, monkeypatch, dt, SMALL_DECODER, key="16bit" + mfma)
    assert place.tensors["grad_value"].dtype == dt
    _mark(_storage_label(mfma), rb, seen=SEEN)


@pytest.mark.parametrize("case", ["value", "grad_out"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("mfma", ["0", "1"])
def test_16bit_decoder_call_with_a_shifted_value_or_grad_out_takes_float32_grad_value(mfma, dtype, case, monkeypatch):
    dt = DTYPES[dtype]
    _, place = decoder_case(case, {"MSDA_SCATTER_MFMA": mfma}, None, monkeypatch, dt, SMALL_DECODER, key="16bit" + mfma)
    assert place.tensors["grad_value"].dtype == torch.float32


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_16bit_decoder_call_with_float32_sampling_tensors(dtype, monkeypatch):
    dt = DTYPES[dtype]
    (rf, rb), place = decoder_case("points", {"MSDA_SCATTER_MFMA": "0"}, None, monkeypatch, dt, SMALL_DECODER, loc32=True, key="loc32")
    assert place.tensors["loc_c"].dtype == torch.float32 and place.tensors["grad_aw_t"].dtype == torch.float32
    assert place.tensors["grad_value"].dtype == dt
    _mark(_storage_label("0"), rb, seen=SEEN)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_a_shifted_grad_value_in_the_storage_type_is_refused_and_not_written(dtype):
    from devis_amd import _native
    dt = DTYPES[dtype]
    r, _ = _decoder_call("tail_gap", dt, *SMALL_DECODER)
    v, lc, ac, lt, at, go = (_t(r[k], dt).contiguous() for k in ("value", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out"))
    shapes, lsi, ftab = _t(r["shapes"]), _t(r["lsi"]), _t(r["ftab"])
    assert _native.grad_value_dtype(v, shapes, lc.shape[1], lc.shape[3], lc.shape[4], clips=1, window=ftab.shape[1], Pt=lt.shape[4],
                                    grad_out=go) == dt
    gv, buf = shifted(torch.full(v.shape, float("nan"), dtype=dt, device=DEV), SHIFTS[dt][0])
    gs = [torch.full_like(x, float("nan")) for x in (lc, ac, lt, at)]
    with pytest.raises(RuntimeError, match="needs grad_value in the arithmetic type"):
        _native.temporal_backward(v, shapes, lsi, ftab, lc, ac, lt, at, go, 1, gv, *gs)
    torch.cuda.synchronize()
    assert bool(gv.isnan().all())
    canaries_intact(buf, SHIFTS[dt][0], gv.numel())


# ---- the resident-window kernels: the encoder call of test_layout_gpu.py --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _encoder_call():
    S0 = int(sum(h * w for h, w in PYR_A))
    r = _rounded(relayout(temporal_case(90, PYR_A, T=2, W=1, Lq=S0, sigma=1.5), "aligned", 37), torch.float32)
    return r, temporal_reference_clips(r, torch.float32)[0]


@pytest.mark.parametrize("case", ["points", "gradients", "points+gradients"])
def test_encoder_call_on_the_window_kernels(case, monkeypatch):
    _env(monkeypatch, {"MSDA_FWD_WIN": "1", "MSDA_BWD_WIN": "1"})
    r, ref = _encoder_call()
    place = Place(shifts_of(case, torch.float32, True))
    got, routes = run_temporal(r, torch.float32, place=place)
    place.check()
    check(got, ref, r, torch.float32)
    routes_as_expected(case, routes, aligned_routes("window", lambda: run_temporal(r, torch.float32)))
    _mark("fwd resident-window", routes[0], seen=SEEN)
    _mark("gather resident-window", routes[1], seen=SEEN)


# ---- matrix-pipe scatter with one coarse level -----------------------------------------------------------------------------------
def test_matrix_pipe_scatter_of_one_level(monkeypatch):
    monkeypatch.setenv("MSDA_SCATTER_MFMA", "1")
    name, pyr, T, W, Lq, label = next(s for s in MFMA_SHAPES if s[0] == "one-small")
    ftab = np.random.default_rng(len(name)).integers(0, T, size=(T, W)).astype(np.int32)
    r = _rounded(relayout(temporal_case(70 + len(name), pyr, T=T, W=W, Lq=Lq, ftab=ftab), "tail_gap", 23), torch.float32)
    place = Place(shifts_of("points", torch.float32, True))
    got, routes = run_temporal(r, torch.float32, place=place)
    place.check()
    check(got, temporal_reference_clips(r, torch.float32)[0], r, torch.float32)
    routes_as_expected("points", routes, run_temporal(r, torch.float32)[1])
    _mark(label, routes[1], seen=SEEN)


# ---- the plain op on the small pyramid: tile, generic, LDS-atomic and global-atomic kernels -------------------------------------
@functools.lru_cache(maxsize=None)
def _plain_call(D, P, dtype=torch.float32):
    r = _rounded(relayout(op_case(10 + D, SMALL, D=D, P=P), "gaps", D), dtype)
    return r, op_reference(r, dtype)


def plain_case(case, env, D, P, monkeypatch, dtype=torch.float32, tol_dtype=None):
    _env(monkeypatch, env)
    r, ref = _plain_call(D, P, dtype)
    place = Place(shifts_of(case, dtype, False))
    got, routes = run_op(r, dtype, place=place)
    place.check()
    check(got, ref, r, tol_dtype or dtype)
    routes_as_expected(case, routes, aligned_routes(("plain", tuple(sorted(env.items())), D, P, dtype), lambda: run_op(r, dtype)))
    return routes


@pytest.mark.parametrize("case", SAME_ROUTE)
@pytest.mark.parametrize("fwd,bwd,env,D", OP_CASES, ids=["%s-D%d" % (f or b, D) for f, b, _, D in OP_CASES])
def test_plain_op_routes_on_shifted_sampling_tensors(fwd, bwd, env, D, case, monkeypatch):
    rf, rb = plain_case(case, env, D, 8 if fwd == "fwd tile, several waves" else 4, monkeypatch)
    if fwd:
        _mark(fwd, rf, seen=SEEN)
    if bwd:
        _mark(bwd, rb, seen=SEEN)


def test_plain_op_with_nothing_16_byte_aligned(monkeypatch):
    """D = 30: value rows of 120 bytes, and every operand and output off alignment by 4, 8 or 12 bytes."""
    env = next(e for f, b, e, D in OP_CASES if f == "fwd generic" and D == 30)
    plain_case("everything", env, 30, 4, monkeypatch)


def test_plain_op_in_float64_with_nothing_16_byte_aligned(monkeypatch):
    """float64 is the generic kernels' alone; every tensor 8 bytes off.  Held to the float32 bars of TOL (there is none for
    float64), against the float64 oracle."""
    plain_case("everything", {}, 32, 4, monkeypatch, torch.float64, tol_dtype=torch.float32)


# ---- autograd -------------------------------------------------------------------------------------------------------------------
def _autograd_call(r, k):
    """MSDeformAttnFunction forward and backward on leaves shifted by k elements (0: aligned); (results, backward routes,
    buffers)."""
    from devis_amd import _native
    from devis_amd.functions import MSDeformAttnFunction
    held, leaves = [], []
    for name in ("value", "loc", "aw"):
        t = _t(r[name], torch.float32)
        if k:
            t, buf = shifted(t, k)
            held.append((buf, k, t.numel(), name))
        leaves.append(t.requires_grad_(True))
    v, loc, aw = leaves
    handed, routes = [], []

    def wrap(orig, bwd):
        def wrapped(*a, **kw):
            handed.extend(x.data_ptr() for x in a if isinstance(x, torch.Tensor))
            orig(*a, **kw)
            if bwd:
                routes.append(_native.last_route())     # (the backward runs on autograd's thread: its route is taken there)
        return wrapped
    with pytest.MonkeyPatch.context() as mp:
        for fn in ("forward", "backward_grads"):
            mp.setattr(_native, fn, wrap(getattr(_native, fn), fn != "forward"))
        out = MSDeformAttnFunction.apply(v, _t(r["shapes"]), _t(r["lsi"]), loc, aw, 2)
        got = (out,) + torch.autograd.grad(out, (v, loc, aw), _t(r["grad_out"], torch.float32))
        torch.cuda.synchronize()
    for x in leaves:            # the host passed the views themselves on, not copies of them
        assert x.data_ptr() in handed and (not k or x.data_ptr() % 16 != 0)
    for buf, kk, n, name in held:
        canaries_intact(buf, kk, n, name)
    return [x.detach() for x in got], routes


@pytest.mark.parametrize("k", SHIFTS[torch.float32])
def test_autograd_function_on_shifted_leaves(k):
    r = _rounded(relayout(op_case(99, SMALL, N=4, M=8, D=32, Lq=31), "tail_gap", 47), torch.float32)
    got, routes = _autograd_call(r, k)
    check([_np(x) for x in got], op_reference(r, torch.float32), r, torch.float32)
    assert len(routes) == 2                             # two im2col_step chunks
    for rb in routes:
        _mark("bwd generic", rb, seen=SEEN)


def test_autograd_function_deterministic_grad_value_has_the_bits_of_the_aligned_call():
    """Under torch.use_deterministic_algorithms(True) grad_value does not depend on the route (README): the
    shifted value takes the generic gather pass, the aligned one the tile kernel."""
    r = _rounded(relayout(op_case(99, SMALL, N=4, M=8, D=32, Lq=31), "tail_gap", 47), torch.float32)
    before = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        want, routes_a = _autograd_call(r, 0)
        got, routes_s = _autograd_call(r, 1)
    finally:
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])
    ref = op_reference(r, torch.float32)
    check([_np(x) for x in want], ref, r, torch.float32)
    check([_np(x) for x in got], ref, r, torch.float32)
    assert len(routes_a) == 2 and len(routes_s) == 2
    assert all("generic kernel" in x for x in routes_s) and not any("generic kernel" in x for x in routes_a), (routes_a, routes_s)
    assert torch.equal(got[1], want[1])


# ---- the mask-head operators: the call on shifted views against the same call on aligned tensors -------------------------------
class Views:
    """Shifted copies of CPU or device tensors, and their canaries."""

    def __init__(self):
        self.held = []

    def __call__(self, t, k):
        if t is None:
            return None
        view, buf = shifted(t.to(DEV), k)
        self.held.append((buf, k, view.numel()))
        return view

    def check(self):
        for buf, k, n in self.held:
            canaries_intact(buf, k, n)


def _same_bits(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), (what, i)
        if a is not None:
            assert a.dtype == b.dtype and torch.equal(a, b), (what, i)


def test_attention_maps_on_shifted_operands_give_the_bits_of_the_aligned_call():
    import devis_amd
    from test_attmap_gpu import grad_out_for, make_inputs
    for dtype in (torch.float32, torch.bfloat16):
        B, Q, n, c, H, W = 3, 7, 8, 32, 13, 21
        q, k, m = make_inputs(B, Q, n, c, H, W, dtype, mask="ragged")
        go = grad_out_for(B, Q, n, H, W, dtype).to(DEV)

        def call(q, k, m):
            q, k = q.requires_grad_(True), k.requires_grad_(True)
            out = devis_amd.attention_maps(q, k, m, num_heads=n)
            return (out.detach(),) + torch.autograd.grad(out, (q, k), go)
        want = call(q.to(DEV), k.to(DEV), m.to(DEV))
        s, views = SHIFTS[dtype], Views()
        got = call(views(q, s[0]), views(k, s[1]), views(m, 3))
        views.check()
        _same_bits(got, want, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_mask_head_stage_on_shifted_operands_gives_the_bits_of_the_aligned_call(dtype):
    import devis_amd
    from test_mhstage_gpu import grad_out_for, make_case
    d = make_case(6, 3, 64, 8, 8, (6, 10), (12, 20), dtype)
    go = grad_out_for(d, dtype)
    names = ("x", "weight", "bias", "skip", "extra")

    def call(t, go):
        t = {k: v.requires_grad_(True) for k, v in t.items()}
        out = devis_amd.mask_head_stage(t["x"], d["G"], t["weight"], t["bias"], skip=t["skip"], skip_index=d["index"].to(DEV),
                                        extra=t["extra"])
        return (out.detach(),) + torch.autograd.grad(out, [t[k] for k in names], go)
    want = call({k: d[k].to(DEV) for k in names}, go.to(DEV))
    s, views = SHIFTS[dtype], Views()
    got = call({k: views(d[k], s[i % 3]) for i, k in enumerate(names)}, views(go, s[2]))
    views.check()
    _same_bits(got, want, dtype)


def test_mask_loss_terms_on_shifted_operands_give_the_bits_of_the_aligned_call():
    import devis_amd
    from test_maskloss_gpu import grads_for, make_case
    src, _ = make_case(3, (9, 11), (30, 41))
    soft = torch.rand(3, 30, 41, generator=torch.Generator().manual_seed(3))
    grads = [g.to(DEV, torch.float32) for g in grads_for(3)]

    def call(s, t):
        s = s.requires_grad_(True)
        focal, dice = devis_amd.mask_loss_terms(s, t, 0.25, 2.0)
        return (focal.detach(), dice.detach()) + torch.autograd.grad([focal, dice], s, grads)
    want = call(src.to(DEV), soft.to(DEV))
    for ks, kt in ((1, 2), (3, 1), (2, 3)):
        views = Views()
        got = call(views(src, ks), views(soft, kt))
        views.check()
        _same_bits(got, want, (ks, kt))


def test_deform_conv2d_on_shifted_operands_gives_the_bits_of_the_aligned_call():
    """Offset, mask, weight and grad_out shifted: out, grad_offset, grad_mask and grad_weight bit for bit, grad_input bit for
    bit under reproducible_grad_input() and against the oracle (float atomics) without it.  mdcn_im2col takes its input and
    its column buffer preallocated, so the one-element-per-lane kernel of a shifted input or column buffer (csrc/mdcn.hip
    vector_width) is run through devis_amd._mdcn directly, against the vector kernel's columns."""
    import devis_amd
    import test_dcn_gpu as T
    from devis_amd import _mdcn
    from devis_amd.functions import deform_conv as D
    tensors, geometry = T.make_inputs(N=3, C=8, Co=5, H=9, W=11, seed=16)
    x, off, w, b, m, g = tensors

    def call(off, w, m, g):
        leaves = [x.to(DEV), off, m, w, b.to(DEV)]
        for t in leaves:
            t.requires_grad_(True)
        out = devis_amd.deform_conv2d(leaves[0], off, w, leaves[4], mask=m, **geometry)
        return [out.detach()] + list(torch.autograd.grad(out, leaves, g))       # NAMES of test_dcn_gpu.py
    aligned = lambda: call(off.to(DEV), w.to(DEV), m.to(DEV), g.to(DEV))        # noqa: E731

    def moved():
        views = Views()
        got = call(views(off, 1), views(w, 2), views(m, 3), views(g, 1))
        views.check()
        return got
    want, got = aligned(), moved()
    _same_bits([got[i] for i in (0, 2, 3, 4)], [want[i] for i in (0, 2, 3, 4)], "out, grad_offset, grad_mask, grad_weight")
    T.assert_close(got, T.oracle(tensors, geometry), T.TOL[torch.float32], "shifted")
    with devis_amd.reproducible_grad_input():
        want, got = aligned(), moved()
    _same_bits(got[:5], want[:5], "reproducible")

    # the native entry point on a shifted input and a shifted column buffer
    xd, od, wd, md = x.to(DEV), off.to(DEV), w.to(DEV), m.to(DEV)
    shape, code, xn, od, md, w2 = D._prepare(xd, od, wd, None, geometry["stride"], geometry["padding"], geometry["dilation"], md)
    assert (shape.C // shape.G) % 4 == 0                # the aligned call takes the 16-byte kernel
    rows, KC = shape.N * shape.Ho * shape.Wo, w2.shape[1]
    cols = torch.full((rows, KC), float("nan"), device=DEV)
    _mdcn.im2col(code, xn, od, md, shape, cols)
    assert bool(cols.isfinite().all())
    for kx, kc in ((1, 0), (0, 2), (3, 1)):
        views = Views()
        xs = views(xn, kx) if kx else xn
        cs = views(torch.full_like(cols, float("nan")), kc) if kc else torch.full_like(cols, float("nan"))
        _mdcn.im2col(code, xs, od, md, shape, cs)
        torch.cuda.synchronize()
        views.check()
        assert torch.equal(cs, cols), (kx, kc)


# ---- every route ---------------------------------------------------------------------------------------------------------------
def test_every_route_was_reached():
    """Runs last: every label of LABELS showed up in msda_last_route() of a passing case
    above.  A case that did not run in this session (a -k selection) is not held against it."""
    missing = sorted(set(LABELS) - SEEN)
    if len(SEEN) < 5:
        pytest.skip("the route cases of this file did not run in this session")
    assert not missing, missing
