"""GPU: every kernel route on level layouts that do not tile [0, S) -- levels with gaps before, between and after them, aligned to
64 rows, in reverse and in random order (include/msda.h: level l occupies rows [lsi[l], lsi[l] + H_l*W_l); gap rows of `value`
are never read and gap rows of grad_value are written as 0).  Gap rows of `value` are NaN, so an output that reads one is not
finite; grad_value is NaN-poisoned before each backward through the C ABI, so a gap row or level row the library does not
write shows up too.  Each case forces its route and asserts, through msda_last_route(), that the route really ran; the last
test asserts that every route of the list below was reached."""
import functools

import numpy as np
import pytest
import torch

from helpers import (LAYOUTS, PYR_A, gaps_zeroed, level_rows, localise, make_inputs, make_temporal_inputs, relayout, round_to,
                     temporal_reference)
from test_op_gpu import _maxabs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: (1e-5, 1e-4), torch.bfloat16: (3e-2, 3e-2), torch.float16: (6e-3, 6e-3)}     # (forward, backward)
TKEYS = ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

# route label -> (substrings that must all be in msda_last_route() of the forward or backward, substrings that must not be)
ROUTES = {
    "fwd tile": (("msda forward (tile kernel)",), ()),
    "fwd tile, several waves": (("msda forward (tile kernel, several waves per tile)",), ()),
    "fwd resident-slab nt1": (("msda forward (resident-slab kernel, 1 tiles per wave)",), ()),
    "fwd resident-slab nt2": (("msda forward (resident-slab kernel, 2 tiles per wave)",), ()),
    "fwd resident-slab nt4": (("msda forward (resident-slab kernel, 4 tiles per wave)",), ()),
    "fwd resident-window": (("msda forward (resident-window kernel",), ()),
    "fwd generic": (("msda forward (generic kernel)",), ()),
    "gather tile": (("msda backward (tile kernel, grad_loc/grad_attn)",), ()),
    "gather resident-slab": (("msda backward (resident-slab kernel, grad_loc/grad_attn)",), ()),
    "gather resident-slab, frame split": (("resident-slab kernel, grad_loc/grad_attn, one source frame per workgroup",), ()),
    "gather resident-window": (("msda backward (resident-window kernel, grad_loc/grad_attn",), ()),
    "bwd generic": (("msda backward (generic kernel)",), ()),
    "scatter owner, level order": (("owner-computes scatter kernel, group-granular)",), ("zero-fill", "matrix-pipe")),
    "scatter owner, image order": (("owner-computes scatter kernel, group-granular, items in image order)",), ("zero-fill", "matrix-pipe")),
    "scatter owner, separate zero-fill": (("owner-computes scatter kernel", "zero-fill of pixels outside the bands"), ()),
    "scatter LDS atomics": (("msda backward (LDS scatter kernel)",), ()),
    "bwd global atomics": (("msda backward (tile kernel, global atomics)",), ()),
    "scatter matrix-pipe NL=1": (("matrix-pipe scatter kernel, coarse levels, 1 level", "owner-computes scatter kernel"), ()),
    "scatter matrix-pipe NL=2": (("matrix-pipe scatter kernel, coarse levels, 2 levels", "owner-computes scatter kernel"), ()),
    "scatter matrix-pipe automatic": (("matrix-pipe scatter kernel, coarse levels, 2 levels",), ()),
    "scatter owner, grad_value in the storage type": (("owner-computes scatter kernel, group-granular, grad_value in the storage type",), ()),
    "scatter matrix-pipe, grad_value in the storage type": (("matrix-pipe scatter kernel, coarse levels, 2 levels, grad_value in the storage type",),
                                                            ()),
    "value only (culling records)": (("msda backward (culling records)",), ("grad_loc/grad_attn",)),
    "sampling only": (("grad_loc/grad_attn",), ("scatter", "culling records")),
    # entry points: the owner-computes scatter (D = 32, <= 4 points) on each of them
    "plain op, im2col_step chunks": (("owner-computes scatter kernel",), ()),
    "temporal, repeated frames": (("owner-computes scatter kernel",), ()),
    "autograd MSDeformAttnFunction": (("owner-computes scatter kernel",), ()),
}
SEEN = set()


def _mark(label, route, seen=SEEN):
    """The route of `label` ran (called once the case's results have passed their checks): it counts as reached."""
    must, must_not = ROUTES[label]
    assert all(s in route for s in must) and not any(s in route for s in must_not), (label, route)
    seen.add(label)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _rounded(d, dtype):
    """Inputs as the kernels see them: rounded once to the storage type (numpy float64 arrays, NaN gaps kept)."""
    d = {k: (np.asarray(v, np.float64) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in d.items()}
    return d if dtype == torch.float64 else round_to(d, dtype)


def op_case(seed, shapes, N=2, M=5, D=32, Lq=37, P=4):
    return make_inputs(seed, N, M, D, Lq, shapes, P, "wide", np.float64, value_scale=1.0)


def temporal_case(seed, shapes, T=6, W=5, M=8, D=32, Lq=300, Pc=4, Pt=4, ftab=None, clips=1, sigma=None):
    ds = []
    for c in range(clips):
        d = make_temporal_inputs(seed + c, T, W, M, D, Lq, shapes, Pc, Pt, ftab=ftab, dtype=np.float64)
        if sigma is not None:
            d["loc_c"] = localise(d["loc_c"], shapes, sigma, seed + 1)
            d["loc_t"] = localise(d["loc_t"], shapes, sigma, seed + 2)
        ds.append(d)
    if clips == 1:
        return ds[0]
    return {k: (np.concatenate([x[k] for x in ds], 0) if k not in ("shapes", "lsi", "ftab") else ds[0][k]) for k in ds[0]}


# ---- runs through the C ABI -----------------------------------------------------------------------------------------------------
def _t(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _np(t):
    return None if t is None else t.double().cpu().numpy()


def _in_place(name, t):
    return t


def run_op(r, dtype, grads=3, step=None, place=_in_place):
    """msda_forward / msda_backward(_grads) on a (relaid) plain call, batch rows in chunks of `step` (the im2col_step loop of
    ms_deform_attn_cuda.cu:61-75).  grad_value starts as NaN.  Returns the outputs and the (forward, backward) routes.
    `place(name, tensor)` returns the tensor the library is handed for operand or output `name` (tests/test_unaligned_gpu.py:
    the same numbers in other memory); by default the tensor itself."""
    from devis_amd import _native
    v, loc, aw, go = (place(k, _t(r[k], dtype).contiguous()) for k in ("value", "loc", "aw", "grad_out"))
    shapes, lsi = _t(r["shapes"]), _t(r["lsi"])
    N, S, M, D = v.shape
    _, Lq, _, L, P, _ = loc.shape
    step = step or N
    out = place("out", torch.full((N, Lq, M * D), float("nan"), dtype=dtype, device=DEV))
    for n in range(0, N, step):
        _native.forward(v[n:n + step], shapes, lsi, loc[n:n + step], aw[n:n + step], out[n:n + step])
    rf = _native.last_route()
    gv = place("grad_value", torch.full(v.shape, float("nan"), device=DEV,
                                        dtype=_native.grad_value_dtype(v[:step], shapes, Lq, L, P, grad_out=go))) if grads & 1 else None
    gl, ga = (place(k, torch.full_like(x, float("nan"))) for k, x in (("grad_loc", loc), ("grad_aw", aw))) if grads & 2 else (None, None)
    c = lambda x, n: None if x is None else x[n:n + step]                  # noqa: E731
    for n in range(0, N, step):
        args = (v[n:n + step], shapes, lsi, loc[n:n + step], aw[n:n + step], go[n:n + step], c(gv, n), c(gl, n), c(ga, n))
        if grads == 3:
            _native.backward(*args)
        else:
            _native.backward_grads(grads, *args)
    rb = _native.last_route()
    torch.cuda.synchronize()
    return [_np(x) for x in (out, gv, gl, ga)], (rf, rb)


def run_temporal(r, dtype, clips=1, grads=3, place=_in_place):
    """msda_temporal_forward / msda_temporal_backward(_grads) on a (relaid) fused temporal call; grad_value starts as NaN.
    `place`: as for run_op."""
    from devis_amd import _native
    v, lc, ac, lt, at, go = (place(k, _t(r[k], dtype).contiguous()) for k in ("value", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out"))
    shapes, lsi, ftab = _t(r["shapes"]), _t(r["lsi"]), _t(r["ftab"])
    G, S, M, D = v.shape
    _, Lq, _, L, Pc, _ = lc.shape
    W, Pt = ftab.shape[1], lt.shape[4]
    out = place("out", torch.full((G, Lq, M * D), float("nan"), dtype=dtype, device=DEV))
    _native.temporal_forward(v, shapes, lsi, ftab, lc, ac, lt, at, clips, out)
    rf = _native.last_route()
    gv = place("grad_value", torch.full(v.shape, float("nan"), device=DEV,
                                        dtype=_native.grad_value_dtype(v, shapes, Lq, L, Pc, clips=clips, window=W, Pt=Pt,
                                                                       grad_out=go))) if grads & 1 else None
    gs = [place("grad_" + k, torch.full_like(x, float("nan")))
          for k, x in (("loc_c", lc), ("aw_c", ac), ("loc_t", lt), ("aw_t", at))] if grads & 2 else [None] * 4
    if grads == 3:
        _native.temporal_backward(v, shapes, lsi, ftab, lc, ac, lt, at, go, clips, gv, *gs)
    else:
        _native.temporal_backward_grads(grads, v, shapes, lsi, ftab, lc, ac, lt, at, go, clips, gv, *gs)
    rb = _native.last_route()
    torch.cuda.synchronize()
    return [_np(x) for x in [out, gv] + gs], (rf, rb)


# ---- the oracle and the checks --------------------------------------------------------------------------------------------------
def op_reference(r, dtype):
    """fp64 oracle on the rounded inputs, gaps zeroed; grad_loc of fp32 runs in fp32 arithmetic (a location on a pixel border in
    fp32 but not in fp64 selects another cell: tests/test_op_gpu.py)."""
    from helpers import oracle_fwd_bwd
    z = gaps_zeroed(r)
    ref = list(oracle_fwd_bwd(z, np.float64))
    if dtype == torch.float32:
        ref[2] = oracle_fwd_bwd(z, np.float32)[2].astype(np.float64)
    return ref


def temporal_reference_clips(r, dtype, clips=1, only=None):
    """Per clip (T frames each) the oracle of the reference's call pattern; `only`: the clips to compute (others None)."""
    z = gaps_zeroed(r)
    T = z["value"].shape[0] // clips
    refs = []
    for c in range(clips):
        if only is not None and c not in only:
            refs.append(None)
            continue
        part = {k: (z[k][c * T:(c + 1) * T] if k not in ("shapes", "lsi", "ftab") else z[k]) for k in TKEYS}
        ref = list(temporal_reference(*(part[k] for k in TKEYS)))
        if dtype == torch.float32:
            ref32 = temporal_reference(*(np.asarray(part[k], np.float32) if part[k].dtype.kind == "f" else part[k] for k in TKEYS))
            ref[2], ref[4] = ref32[2].astype(np.float64), ref32[4].astype(np.float64)
        refs.append(ref)
    return refs


def check(got, ref, r, dtype, rows=slice(None)):
    """Forward and gradients against the oracle (the suite's tolerances, relative to the max), everything finite, the level rows
    of grad_value against the oracle's, the gap rows exactly 0.  `rows`: the batch rows of `got` that `ref` covers."""
    tf, tb = TOL[dtype]
    scale = lambda x: max(1.0, float(np.abs(x).max()))                     # noqa: E731
    for i, (a, b) in enumerate(zip(got, ref)):
        if a is None:
            continue
        a = a[rows]
        assert np.isfinite(a).all(), ("not finite", i)
        if i == 1:
            lv, lr = level_rows(a, r), level_rows(b, r)
            assert _maxabs(lv, lr) <= tb * scale(lr), ("grad_value level rows", _maxabs(lv, lr))
            assert (a[:, r["gap"]] == 0).all(), "grad_value gap rows"
        else:
            tol = tf if i == 0 else tb
            assert _maxabs(a, b) <= tol * scale(b), (i, _maxabs(a, b), scale(b))


def _env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---- forward and gather-pass routes: the plain op on a small pyramid, D in {32, 30, 64}, M = 5 ---------------------------------
SMALL = [(9, 11), (6, 10), (4, 5), (2, 3)]
TILE = {"MSDA_FWD_RS": "0", "MSDA_FWD_WIN": "0", "MSDA_BWD_RS": "0", "MSDA_BWD_WIN": "0"}
OP_ROUTES = [
    # label of the forward, label of the backward, knobs, channel counts (the tile kernels take D a multiple of 4)
    ("fwd tile", "gather tile", dict(TILE, MSDA_FWD_TILE_WAVES="1"), (32, 64)),
    ("fwd tile, several waves", None, dict(TILE, MSDA_FWD_TILE_WAVES="2"), (32,)),       # (G = 4 / 8 lanes per row, >= 2 chunks)
    ("fwd generic", "bwd generic", {"MSDA_FORCE_GENERIC": "1"}, (32, 30, 64)),
    (None, "scatter LDS atomics", {"MSDA_SCATTER_OWN": "0"}, (32,)),
    (None, "bwd global atomics", {"MSDA_BWD_MODE": "atomic"}, (32, 64)),
]
OP_CASES = [(f, b, e, D) for f, b, e, Ds in OP_ROUTES for D in Ds]


@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("fwd,bwd,env,D", OP_CASES, ids=["%s-D%d" % (f or b, D) for f, b, _, D in OP_CASES])
def test_plain_op_routes(fwd, bwd, env, D, kind, monkeypatch):
    _env(monkeypatch, env)
    d = op_case(10 + D, SMALL, D=D, P=8 if fwd == "fwd tile, several waves" else 4)     # (waves share the 16-point chunks)
    r = _rounded(relayout(d, kind, D), torch.float32)
    got, (rf, rb) = run_op(r, torch.float32)
    check(got, op_reference(r, torch.float32), r, torch.float32)
    if fwd:
        _mark(fwd, rf)
    if bwd:
        _mark(bwd, rb)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("fwd,bwd,env", [r[:3] for r in OP_ROUTES[:3]], ids=[r[0] for r in OP_ROUTES[:3]])
def test_plain_op_routes_16bit(fwd, bwd, env, dtype, monkeypatch):
    _env(monkeypatch, env)
    dt = DTYPES[dtype]
    r = _rounded(relayout(op_case(21, SMALL, M=3, P=8), "shuffled", 4), dt)
    got, (rf, rb) = run_op(r, dt)
    check(got, op_reference(r, dt), r, dt)
    _mark(fwd, rf)
    if bwd:
        _mark(bwd, rb)


def test_plain_op_separate_zero_fill_for_a_level_wider_than_a_band(monkeypatch):
    """A level of 1100 pixels per row takes the float-atomic branch: grad_value is zero-filled by its own launch, which must
    zero the gap rows and leave the level rows to the scatter."""
    for kind in LAYOUTS:
        d = op_case(31, [(2, 1100), (3, 5)], N=1, M=2, Lq=23)
        r = _rounded(relayout(d, kind, 9), torch.float32)
        got, (rf, rb) = run_op(r, torch.float32)
        check(got, op_reference(r, torch.float32), r, torch.float32)
        _mark("scatter owner, separate zero-fill", rb)


@pytest.mark.parametrize("kind", LAYOUTS)
def test_plain_op_im2col_step_chunks(kind):
    d = op_case(41, SMALL, N=4, M=8, D=32, Lq=29)
    r = _rounded(relayout(d, kind, 13), torch.float32)
    got, (rf, rb) = run_op(r, torch.float32, step=2)
    check(got, op_reference(r, torch.float32), r, torch.float32)
    _mark("plain op, im2col_step chunks", rb)


# ---- the decoder call of DeVIS: fused temporal op on the 360x640 pyramid, 6 frames, 300 queries --------------------------------
DEC_ROUTES = [
    # forward label, backward labels, knobs, pins
    ("fwd resident-slab nt1", ("gather resident-slab", "scatter owner, level order"),
     {"MSDA_FWD_RS": "1", "MSDA_FWD_RS_NT": "1", "MSDA_BWD_RS": "1", "MSDA_BWD_RS_FSPLIT": "0", "MSDA_SCATTER_MFMA": "0"},
     {"scatter_order": 1}),
    ("fwd resident-slab nt2", ("gather resident-slab, frame split", "scatter owner, image order"),
     {"MSDA_FWD_RS": "1", "MSDA_FWD_RS_NT": "2", "MSDA_BWD_RS": "1", "MSDA_BWD_RS_FSPLIT": "2", "MSDA_SCATTER_MFMA": "0"},
     {"scatter_order": 2}),
    ("fwd resident-slab nt4", ("scatter matrix-pipe NL=2",), {"MSDA_FWD_RS": "1", "MSDA_FWD_RS_NT": "4", "MSDA_SCATTER_MFMA": "1"}, {}),
    ("fwd tile", ("gather tile",), {"MSDA_FWD_RS": "0", "MSDA_FWD_WIN": "0", "MSDA_BWD_RS": "0", "MSDA_BWD_WIN": "0"}, {}),
]


def _pin(r, pins, clips=1):
    """Pin `pins` for the backward key of this call; returns the key (to unpin)."""
    from devis_amd import _native
    G, S, M, D = r["value"].shape
    L, W = len(r["shapes"]), r["ftab"].shape[1]
    key = _native.route_key(True, 0, clips, G // clips, W, S, M, D, L, r["loc_c"].shape[1], r["loc_c"].shape[4],
                            r["loc_t"].shape[4], r["shapes"])
    _native.pin_route(key, pins)
    return key


@functools.lru_cache(maxsize=None)
def _decoder_call(kind, dtype, T=6, Lq=300):
    """The decoder call on layout `kind` and its oracle, made once for all the routes that run it."""
    r = _rounded(relayout(temporal_case(51, PYR_A, T=T, W=T - 1, Lq=Lq), kind, 17), dtype)
    refs = temporal_reference_clips(r, dtype)
    return r, refs[0]


@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("fwd,bwd,env,pins", DEC_ROUTES, ids=[a for a, *_ in DEC_ROUTES])
def test_decoder_call_routes(fwd, bwd, env, pins, kind, monkeypatch):
    from devis_amd import _native
    _env(monkeypatch, env)
    r, ref = _decoder_call(kind, torch.float32)
    key = _pin(r, pins) if pins else None
    try:
        got, (rf, rb) = run_temporal(r, torch.float32)
    finally:
        if key:
            _native.pin_route(key, "")
    check(got, ref, r, torch.float32)
    _mark(fwd, rf)
    for b in bwd:
        _mark(b, rb)


@pytest.mark.parametrize("kind", ["gaps", "tail_gap", "reversed"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("mfma", ["0", "1"])
def test_decoder_call_grad_value_in_the_storage_type(mfma, dtype, kind, monkeypatch):
    """16-bit value, D = 32, 4 points: the owner-computes (and matrix-pipe) scatter write grad_value in the storage type."""
    monkeypatch.setenv("MSDA_SCATTER_MFMA", mfma)
    dt = DTYPES[dtype]
    r, ref = _decoder_call(kind, dt, T=4, Lq=100)
    got, (rf, rb) = run_temporal(r, dt)
    check(got, ref, r, dt)
    _mark("scatter matrix-pipe, grad_value in the storage type" if mfma == "1" else "scatter owner, grad_value in the storage type", rb)


# ---- the matrix-pipe scatter: the small pyramids of test_mfma_gpu.py, forced, and the 4-clip batch that takes it by itself -----
MFMA_SHAPES = [
    ("two-small", [(9, 11), (6, 10), (4, 5)], 4, 3, 41, "scatter matrix-pipe NL=2"),
    ("three", [(7, 9), (5, 6), (3, 4)], 5, 4, 23, "scatter matrix-pipe NL=2"),
    ("one-small", [(30, 30), (20, 19), (5, 4)], 3, 2, 50, "scatter matrix-pipe NL=1"),
    ("A", PYR_A, 3, 2, 37, "scatter matrix-pipe NL=2"),
]


@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,pyr,T,W,Lq,label", MFMA_SHAPES, ids=[s[0] for s in MFMA_SHAPES])
def test_matrix_pipe_scatter_forced(name, pyr, T, W, Lq, label, dtype, kind, monkeypatch):
    monkeypatch.setenv("MSDA_SCATTER_MFMA", "1")
    dt = DTYPES[dtype]
    ftab = np.random.default_rng(len(name)).integers(0, T, size=(T, W)).astype(np.int32)      # repeated and missing frames
    r = _rounded(relayout(temporal_case(70 + len(name), pyr, T=T, W=W, Lq=Lq, ftab=ftab), kind, 23), dt)
    got, (rf, rb) = run_temporal(r, dt)
    check(got, temporal_reference_clips(r, dt)[0], r, dt)
    _mark(label, rb)


@pytest.mark.parametrize("kind", ["tail_gap"])
def test_matrix_pipe_scatter_automatic_on_the_bench_batch(kind, route_rules_only, monkeypatch):
    """The headline call batched (4 clips x 6 frames x 8 heads = 192 items, as in test_mfma_gpu.py): the route rules put the two
    coarse levels on the matrix pipe by themselves."""
    monkeypatch.delenv("MSDA_SCATTER_MFMA", raising=False)
    clips = 4
    r = _rounded(relayout(temporal_case(80, PYR_A, clips=clips), kind, 29), torch.float32)
    got, (rf, rb) = run_temporal(r, torch.float32, clips=clips)
    assert np.isfinite(got[1]).all() and (got[1][:, r["gap"]] == 0).all()
    refs = temporal_reference_clips(r, torch.float32, clips, only=(0, clips - 1))
    for c in (0, clips - 1):
        check(got, refs[c], r, torch.float32, rows=slice(c * 6, (c + 1) * 6))
    _mark("scatter matrix-pipe automatic", rb)


@pytest.mark.parametrize("kind", ["tail_gap", "gaps", "reversed"])
def test_matrix_pipe_stale_hint_fills_the_hidden_levels_own_rows_with_nan(kind):
    """The stale-hint case of test_mfma_gpu.py with two hidden levels (NL = 2) and a gap between them: the NaN fill covers the
    two levels' own rows of grad_value, not the gap, and nothing else of it."""
    import ctypes
    import os
    from devis_amd import _native
    lib = _native.load()
    real = [(10, 12), (9, 10), (19, 20)]                  # the hint claims (6, 10), (4, 5) for the last two: 80 px, NL = 2
    d = make_inputs(5, 2, 8, 32, 40, real, 4, "unit", np.float32, value_scale=1.0)
    r = relayout(d, kind, 31)
    t = {k: _t(r[k]) for k in ("value", "shapes", "lsi", "loc", "aw", "grad_out")}
    N, S, M, D = t["value"].shape
    _, Lq, _, L, P, _ = t["loc"].shape
    gv = torch.full(t["value"].shape, float("nan"), device=DEV)
    gl, ga = torch.empty_like(t["loc"]), torch.empty_like(t["aw"])
    ws = _native.bwd_workspace(DEV, N, Lq, M, L)
    lie = (ctypes.c_int64 * 6)(10, 12, 6, 10, 4, 5)
    os.environ["MSDA_SCATTER_MFMA"] = "1"
    _native.reload_knobs()
    try:
        rc = lib.msda_backward(0, t["value"].data_ptr(), t["shapes"].data_ptr(), t["lsi"].data_ptr(), t["loc"].data_ptr(),
                               t["aw"].data_ptr(), t["grad_out"].data_ptr(), N, S, M, D, L, Lq, P, gv.data_ptr(), 0,
                               gl.data_ptr(), ga.data_ptr(), ws.data_ptr(), ws.numel() * 4, None, lie,
                               torch.cuda.current_stream().cuda_stream)
        route = _native.last_route()
    finally:
        os.environ.pop("MSDA_SCATTER_MFMA", None)
        _native.reload_knobs()
    assert rc == 0, route
    torch.cuda.synchronize()
    g = gv.cpu().numpy()
    lsi = r["lsi"]
    hidden = np.zeros(S, dtype=bool)
    for l in (1, 2):
        hidden[lsi[l]:lsi[l] + real[l][0] * real[l][1]] = True
    assert np.isnan(g[:, hidden]).all(), kind
    assert not np.isnan(g[:, ~hidden]).any(), kind
    assert (g[:, r["gap"]] == 0).all(), kind
    assert "matrix-pipe scatter kernel, coarse levels, 2 levels" in route, route


# ---- the resident-window kernels: one encoder-shaped clip of the 360x640 pyramid (Lq = sum H*W, now != S) ----------------------
@pytest.mark.parametrize("kind", ["aligned", "reversed"])
def test_encoder_call_on_the_window_kernels(kind, monkeypatch):
    monkeypatch.setenv("MSDA_FWD_WIN", "1")
    monkeypatch.setenv("MSDA_BWD_WIN", "1")
    S0 = int(sum(h * w for h, w in PYR_A))
    r = _rounded(relayout(temporal_case(90, PYR_A, T=2, W=1, Lq=S0, sigma=1.5), kind, 37), torch.float32)
    assert r["value"].shape[1] != S0
    got, (rf, rb) = run_temporal(r, torch.float32)
    check(got, temporal_reference_clips(r, torch.float32)[0], r, torch.float32)
    _mark("fwd resident-window", rf)
    _mark("gather resident-window", rb)


# ---- gradient subsets, windows with repeated frames, autograd --------------------------------------------------------------------
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("grads", [1, 2], ids=["value", "sampling"])
def test_gradient_subsets(grads, kind):
    r = _rounded(relayout(temporal_case(95, [(12, 20), (6, 10), (3, 5)], T=4, W=3, Lq=60), kind, 41), torch.float32)
    got, (rf, rb) = run_temporal(r, torch.float32, grads=grads)
    assert (got[1] is None) == (grads == 2) and (got[2] is None) == (grads == 1)
    check(got, temporal_reference_clips(r, torch.float32)[0], r, torch.float32)
    _mark("value only (culling records)" if grads == 1 else "sampling only", rb)


@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_temporal_windows_with_repeated_frames(dtype, kind):
    ftab = np.array([[1, 1], [0, 2], [1, 3], [2, 4], [3, 3]], dtype=np.int32)
    dt = DTYPES[dtype]
    r = _rounded(relayout(temporal_case(97, [(9, 7), (5, 4), (3, 2)], T=5, W=2, Lq=45, Pt=2, ftab=ftab), kind, 43), dt)
    got, (rf, rb) = run_temporal(r, dt)
    check(got, temporal_reference_clips(r, dt)[0], r, dt)
    _mark("temporal, repeated frames", rb)


@pytest.mark.parametrize("kind", ["reversed", "tail_gap"])
def test_autograd_function_on_a_relaid_call(kind):
    """MSDeformAttnFunction: grad_value comes from torch.empty (functions/ms_deform_attn_func.py), so its gap rows are zero only
    because the library wrote them."""
    from devis_amd.functions import MSDeformAttnFunction
    from test_mfma_gpu import _routes_of_backward
    r = _rounded(relayout(op_case(99, SMALL, N=4, M=8, D=32, Lq=31), kind, 47), torch.float32)
    v, loc, aw = (_t(r[k], torch.float32).requires_grad_(True) for k in ("value", "loc", "aw"))

    def fwd_bwd():
        out = MSDeformAttnFunction.apply(v, _t(r["shapes"]), _t(r["lsi"]), loc, aw, 2)
        return (out,) + torch.autograd.grad(out, (v, loc, aw), _t(r["grad_out"], torch.float32))
    got, routes = _routes_of_backward(fwd_bwd)          # (the backward runs on autograd's thread: its route is taken there)
    torch.cuda.synchronize()
    check([_np(x.detach()) for x in got], op_reference(r, torch.float32), r, torch.float32)
    assert len(routes) == 2                             # two im2col_step chunks
    for rb in routes:
        _mark("autograd MSDeformAttnFunction", rb)


def test_every_route_was_reached():
    """Runs last: every route of ROUTES showed up in msda_last_route() of a passing case above.  A case that did not run in this
    session (a -k selection) is not held against it."""
    missing = sorted(set(ROUTES) - SEEN)
    if len(SEEN) < 5:
        pytest.skip("the route cases of this file did not run in this session")
    assert not missing, missing
