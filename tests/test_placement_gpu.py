"""GPU: every kernel route on sampling locations and attention weights that random draws do not produce (helpers.place): pixel
coordinates exactly on integers, on and next to the excluded ends -1 and H, NaN / inf / huge locations, queries, levels, frames
and whole calls without a point in range, points piled on one cell, zero, negative and unnormalised weights.  Every route restates
the reference's range test, floor and corner validity, and the backward hands culling records from the gather pass to the scatter
pass: these are the inputs on which the copies can disagree.  tests/test_placement_cpu.py shows that the oracle has one answer for
them.  The routes, their forcing and the runs through the C ABI (gradients start as NaN) are those of tests/test_layout_gpu.py.

Per case: forward and gradients against the fp64 oracle on the rounded inputs with the suite's tolerances (grad_loc of f32 runs
against the fp32-arithmetic oracle; for on_grid / edges, whose coordinates are exact in every arithmetic, the placed points'
grad_loc against the fp64 oracle too); everything finite; grad_loc / grad_attn exactly 0 at every point placed out of range,
grad_loc exactly 0 at weight 0; grad_value exactly 0 on what all_out emptied; and with every out-of-range location replaced by -10
the forward, grad_loc and grad_attn keep their bits.  grad_value then keeps its bits where its sums have a fixed order (the matrix-
pipe levels, the deterministic mode); the owner-computes lists are linked in arrival order and the other scatters use atomics
(tests/test_mfma_gpu.py: last-bit differences from run to run, more where many terms meet on one pixel), so elsewhere the moved
call's grad_value is held to the suite's backward tolerance."""
import functools

import numpy as np
import pytest
import torch

from helpers import POW2, POW2_4, PYR_A, oracle_fwd_bwd, out_moved, place, round_to, temporal_reference
from test_layout_gpu import (DEC_ROUTES, DEV, DTYPES, MFMA_SHAPES, OP_CASES, OP_ROUTES, ROUTES, SMALL, TKEYS, TOL, _env, _np, _pin,
                             _rounded, _t, check, op_case, run_op, run_temporal, temporal_case)
from test_layout_gpu import _mark as _layout_mark
from test_op_gpu import _maxabs

pytestmark = pytest.mark.gpu

SEEN = set()
KINDS = ("on_grid", "edges", "nonfinite", "huge", "all_out", "all_out_call", "piled", "weights")
CORE = ("edges", "nonfinite", "all_out")                      # the kinds every route keeps where the product is thinned
EXACT = ("on_grid", "edges")                                  # take power-of-two pyramids


def _mark(label, route):
    _layout_mark(label, route, SEEN)


def _pyr(kind, odd, pow2):
    return pow2 if kind in EXACT else odd


# ---- inputs, oracle, checks -----------------------------------------------------------------------------------------------------
def placed(d, kind, seed, dtype, loc32=False):
    """(call rounded to the storage type -- locations and weights to float32 with `loc32` --, masks)."""
    p, m = place(d, "all_out", seed, whole=True) if kind == "all_out_call" else place(d, kind, seed)
    r = _rounded(p, dtype)
    if loc32:
        for k in p:
            if k.startswith(("loc", "aw")):
                r[k] = round_to({k: np.asarray(p[k], np.float64)}, torch.float32)[k]
    r["gap"] = np.zeros(r["value"].shape[1], dtype=bool)
    return r, m


def reference(r, dtype):
    """(fp64 oracle, with the fp32-arithmetic grad_loc for an f32 run; the fp64 grad_loc by location key)."""
    temporal = "ftab" in r
    if temporal:
        fn = lambda t: temporal_reference(*(np.asarray(r[k], t) if r[k].dtype.kind == "f" else r[k] for k in TKEYS))    # noqa: E731
    else:
        fn = lambda t: oracle_fwd_bwd(r, t)                                                                                # noqa: E731
    ref = list(fn(np.float64))
    gl = (2, 4) if temporal else (2,)
    gl64 = [ref[i] for i in gl]
    if dtype == torch.float32:
        r32 = fn(np.float32)
        for i in gl:
            ref[i] = r32[i].astype(np.float64)
    return ref, gl64


def verify(got, ref, gl64, r, m, dtype, kind):
    check(got, ref, r, dtype)                                  # the tolerances of TOL, every output finite
    tb = TOL[dtype][1]
    keys = ("loc_c", "loc_t") if "ftab" in r else ("loc",)
    for j, lk in enumerate(keys):
        gl, ga = got[2 + 2 * j], got[3 + 2 * j]
        if gl is None:
            continue
        out, zw, pl = m["out"][lk], m["zero_w"][lk], m["placed"][lk]
        assert (gl[out] == 0).all() and (ga[out] == 0).all(), (lk, "gradients of a point out of range")
        assert (gl[zw] == 0).all(), (lk, "grad_loc at weight 0")
        if kind in EXACT:
            err = _maxabs(gl[pl], gl64[j][pl])
            assert err <= tb * max(1.0, float(np.abs(gl64[j]).max())), (lk, "grad_loc of the placed points against fp64", err)
    gv = got[1]
    if gv is not None:
        for l in m["levels"]:
            H, W = r["shapes"][l]
            assert (gv[:, r["lsi"][l]:r["lsi"][l] + H * W] == 0).all(), ("grad_value of the emptied level", l)
        if m["frames"]:
            assert (gv[m["frames"]] == 0).all(), "grad_value of the emptied frame"
        if m["call"]:
            assert (gv == 0).all(), "grad_value of a call without a point in range"
    if m["call"]:
        assert (got[0] == 0).all()


def verify_moved(got, moved, r, dtype, bits_of_grad_value="none", sampling_bits=True):
    """The same call with every out-of-range location at (-10, -10)."""
    for i, (a, b) in enumerate(zip(got, moved)):
        if a is None:
            continue
        if i == 1 and bits_of_grad_value != "all":
            assert _maxabs(a, b) <= TOL[dtype][1] * max(1.0, float(np.abs(b).max())), "grad_value moved"
            if bits_of_grad_value == "last two levels":
                s = int(np.sort(r["lsi"])[-2])
                assert np.array_equal(a[:, s:], b[:, s:]), "grad_value of the matrix-pipe levels changed bits"
        elif i >= 2 and not sampling_bits:
            assert _maxabs(a, b) <= TOL[dtype][1] * max(1.0, float(np.abs(b).max())), i
        else:
            assert np.array_equal(a, b), ("bits changed with the out-of-range locations", i)


def _gv_bits(*routes):
    r = " ".join(routes)
    return "all" if "fixed-point" in r else "last two levels" if "coarse levels, 2 levels" in r else "none"


def run_case(d, kind, seed, dtype, run, sampling_bits=True):
    """Place, run, check against the oracle and against the moved call; returns the routes."""
    r, m = placed(d, kind, seed, dtype)
    ref, gl64 = reference(r, dtype)
    got, (rf, rb) = run(r)
    verify(got, ref, gl64, r, m, dtype, kind)
    if any(x.any() for x in m["out"].values()):
        moved, (rf2, rb2) = run(out_moved(r, m))
        assert (rf2, rb2) == (rf, rb)
        verify_moved(got, moved, r, dtype, _gv_bits(rb), sampling_bits)
    return rf, rb


# ---- the plain op: tile, generic, LDS-atomic and global-atomic routes ----------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fwd,bwd,env,D", OP_CASES, ids=["%s-D%d" % (f or b, D) for f, b, _, D in OP_CASES])
def test_plain_op_routes(fwd, bwd, env, D, kind, monkeypatch):
    _env(monkeypatch, env)
    d = op_case(110 + D, _pyr(kind, SMALL, POW2), D=D, P=8 if fwd == "fwd tile, several waves" else 4)
    loose = bwd in ("bwd generic", "bwd global atomics")
    rf, rb = run_case(d, kind, D, torch.float32, lambda r: run_op(r, torch.float32), sampling_bits=not loose)
    if fwd:
        _mark(fwd, rf)
    if bwd:
        _mark(bwd, rb)


def _run_op_loc32(r, dtype):
    """run_op with float32 locations and weights beside a 16-bit value."""
    from devis_amd import _native
    v, go = (_t(r[k], dtype).contiguous() for k in ("value", "grad_out"))
    loc, aw = (_t(r[k], torch.float32).contiguous() for k in ("loc", "aw"))
    shapes, lsi = _t(r["shapes"]), _t(r["lsi"])
    N, Lq, M, L, P, _ = loc.shape
    out = torch.full((N, Lq, M * v.shape[3]), float("nan"), dtype=dtype, device=DEV)
    _native.forward(v, shapes, lsi, loc, aw, out)
    rf = _native.last_route()
    gv = torch.full(v.shape, float("nan"), device=DEV, dtype=_native.grad_value_dtype(v, shapes, Lq, L, P, grad_out=go))
    gl, ga = torch.full_like(loc, float("nan")), torch.full_like(aw, float("nan"))
    _native.backward(v, shapes, lsi, loc, aw, go, gv, gl, ga)
    rb = _native.last_route()
    torch.cuda.synchronize()
    return [_np(x) for x in (out, gv, gl, ga)], (rf, rb)


@pytest.mark.parametrize("kind", CORE + ("huge",))
@pytest.mark.parametrize("dtype,loc32", [("bf16", False), ("f16", False), ("bf16", True), ("f16", True)],
                         ids=["bf16", "f16", "bf16_loc32", "f16_loc32"])
@pytest.mark.parametrize("fwd,bwd,env", [r[:3] for r in OP_ROUTES[:3]], ids=[r[0] for r in OP_ROUTES[:3]])
def test_plain_op_routes_16bit(fwd, bwd, env, dtype, loc32, kind, monkeypatch):
    _env(monkeypatch, env)
    dt = DTYPES[dtype]
    d = op_case(121, _pyr(kind, SMALL, POW2), M=3, P=8)
    r, m = placed(d, kind, 5, dt, loc32)
    ref, gl64 = reference(r, dt)
    run = (lambda x: _run_op_loc32(x, dt)) if loc32 else (lambda x: run_op(x, dt))
    got, (rf, rb) = run(r)
    verify(got, ref, gl64, r, m, dt, kind)
    moved, _ = run(out_moved(r, m))
    verify_moved(got, moved, r, dt, sampling_bits=bwd != "bwd generic")
    _mark(fwd, rf)
    if bwd:
        _mark(bwd, rb)


@pytest.mark.parametrize("kind", [k for k in KINDS if k != "on_grid"])          # (on_grid walks every column: 64 at most)
def test_plain_op_separate_zero_fill_for_a_level_wider_than_a_band(kind):
    d = op_case(131, _pyr(kind, [(2, 1100), (3, 5)], [(2, 2048), (4, 4)]), N=1, M=2, Lq=23)
    rf, rb = run_case(d, kind, 9, torch.float32, lambda r: run_op(r, torch.float32))
    _mark("scatter owner, separate zero-fill", rb)


@pytest.mark.parametrize("kind", CORE)
def test_plain_op_im2col_step_chunks(kind):
    d = op_case(141, _pyr(kind, SMALL, POW2), N=4, M=8, D=32, Lq=29)
    rf, rb = run_case(d, kind, 13, torch.float32, lambda r: run_op(r, torch.float32, step=2))
    _mark("plain op, im2col_step chunks", rb)


@pytest.mark.parametrize("kind", CORE)
def test_autograd_function(kind):
    from devis_amd.functions import MSDeformAttnFunction
    from test_mfma_gpu import _routes_of_backward
    r, m = placed(op_case(199, _pyr(kind, SMALL, POW2), N=4, M=8, D=32, Lq=31), kind, 47, torch.float32)
    ref, gl64 = reference(r, torch.float32)
    v, loc, aw = (_t(r[k], torch.float32).requires_grad_(True) for k in ("value", "loc", "aw"))

    def fwd_bwd():
        out = MSDeformAttnFunction.apply(v, _t(r["shapes"]), _t(r["lsi"]), loc, aw, 2)
        return (out,) + torch.autograd.grad(out, (v, loc, aw), _t(r["grad_out"], torch.float32))
    got, routes = _routes_of_backward(fwd_bwd)
    torch.cuda.synchronize()
    verify([_np(x.detach()) for x in got], ref, gl64, r, m, torch.float32, kind)
    for rb in routes:
        _mark("autograd MSDeformAttnFunction", rb)


# ---- the decoder call: 6 frames, 300 queries, the 360x640 pyramid (power-of-two levels for the exact kinds) --------------------
@functools.lru_cache(maxsize=None)
def _decoder_call(kind, dtype, T=6, Lq=300):
    r, m = placed(temporal_case(151, _pyr(kind, PYR_A, POW2_4), T=T, W=T - 1, Lq=Lq), kind, 17, dtype)
    return (r, m) + reference(r, dtype)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fwd,bwd,env,pins", DEC_ROUTES, ids=[a for a, *_ in DEC_ROUTES])
def test_decoder_call_routes(fwd, bwd, env, pins, kind, monkeypatch):
    from devis_amd import _native
    _env(monkeypatch, env)
    r, m, ref, gl64 = _decoder_call(kind, torch.float32)
    key = _pin(r, pins) if pins else None
    try:
        got, (rf, rb) = run_temporal(r, torch.float32)
        moved, _ = run_temporal(out_moved(r, m), torch.float32)
    finally:
        if key:
            _native.pin_route(key, "")
    verify(got, ref, gl64, r, m, torch.float32, kind)
    verify_moved(got, moved, r, torch.float32, _gv_bits(rb))
    _mark(fwd, rf)
    for b in bwd:
        _mark(b, rb)


@pytest.mark.parametrize("kind", CORE)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("mfma", ["0", "1"])
def test_decoder_call_grad_value_in_the_storage_type(mfma, dtype, kind, monkeypatch):
    monkeypatch.setenv("MSDA_SCATTER_MFMA", mfma)
    dt = DTYPES[dtype]
    r, m, ref, gl64 = _decoder_call(kind, dt, T=4, Lq=100)
    got, (rf, rb) = run_temporal(r, dt)
    verify(got, ref, gl64, r, m, dt, kind)
    _mark("scatter matrix-pipe, grad_value in the storage type" if mfma == "1" else "scatter owner, grad_value in the storage type", rb)


# ---- the matrix-pipe scatter, forced on small pyramids and by itself on the 4-clip batch ----------------------------------------
MFMA_POW2 = {"two-small": [(8, 16), (4, 8), (2, 4)], "three": [(8, 8), (4, 8), (2, 4)], "one-small": [(32, 32), (16, 32), (4, 4)],
             "A": POW2_4}
MFMA_CASES = [(s, "f32", k) for s in MFMA_SHAPES for k in KINDS] + [(s, "bf16", k) for s in MFMA_SHAPES for k in CORE]


@pytest.mark.parametrize("shape,dtype,kind", MFMA_CASES, ids=["%s-%s-%s" % (s[0], t, k) for s, t, k in MFMA_CASES])
def test_matrix_pipe_scatter_forced(shape, dtype, kind, monkeypatch):
    name, pyr, T, W, Lq, label = shape
    monkeypatch.setenv("MSDA_SCATTER_MFMA", "1")
    dt = DTYPES[dtype]
    ftab = np.random.default_rng(len(name)).integers(0, T, size=(T, W)).astype(np.int32)      # repeated and missing frames
    d = temporal_case(170 + len(name), _pyr(kind, pyr, MFMA_POW2[name]), T=T, W=W, Lq=Lq, ftab=ftab)
    rf, rb = run_case(d, kind, 23, dt, lambda r: run_temporal(r, dt))
    _mark(label, rb)


@pytest.mark.parametrize("kind", CORE)
def test_matrix_pipe_scatter_automatic_on_the_bench_batch(kind, route_rules_only, monkeypatch):
    monkeypatch.delenv("MSDA_SCATTER_MFMA", raising=False)
    clips, T = 4, 6
    r, m = placed(temporal_case(180, _pyr(kind, PYR_A, POW2_4), clips=clips), kind, 29, torch.float32)
    got, (rf, rb) = run_temporal(r, torch.float32, clips=clips)
    for c in (0, clips - 1):                                   # the oracle of the first and the last clip
        rows = slice(c * T, (c + 1) * T)
        part = {k: (v[rows] if isinstance(v, np.ndarray) and k not in ("shapes", "lsi", "ftab", "gap") else v) for k, v in r.items()}
        pm = {k: ({a: b[rows] for a, b in v.items()} if isinstance(v, dict) else v) for k, v in m.items()}
        pm["frames"] = [f - c * T for f in m["frames"] if c * T <= f < (c + 1) * T]
        ref, gl64 = reference(part, torch.float32)
        verify([x[rows] for x in got], ref, gl64, part, pm, torch.float32, kind)
    moved, _ = run_temporal(out_moved(r, m), torch.float32, clips=clips)
    verify_moved(got, moved, r, torch.float32, _gv_bits(rb))
    _mark("scatter matrix-pipe automatic", rb)


# ---- an encoder-shaped call (one query per pixel) on the resident-window kernels; >= 2048 queries: the culling records' block
# ---- summaries are written and read, and nonfinite / all_out empty two whole blocks of 64 queries -------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_encoder_call_on_the_window_kernels_and_the_cull_summary(kind, monkeypatch):
    monkeypatch.setenv("MSDA_FWD_WIN", "1")
    monkeypatch.setenv("MSDA_BWD_WIN", "1")
    pyr = _pyr(kind, PYR_A, POW2_4)
    S0 = int(sum(h * w for h, w in pyr))
    assert S0 >= 2048                                          # (msda_api.hip: block summaries from 2048 queries on)
    d = temporal_case(190, pyr, T=2, W=1, Lq=S0, sigma=1.5)
    r, m = placed(d, kind, 37, torch.float32)
    if kind in ("nonfinite", "all_out"):
        whole = m["out"]["loc_c"].all(axis=(2, 3, 4)) & m["out"]["loc_t"].all(axis=(2, 3, 4))          # [frames, Lq]
        assert any(whole[:, b:b + 64].all() for b in range(0, S0 - 63, 64))
    ref, gl64 = reference(r, torch.float32)
    got, (rf, rb) = run_temporal(r, torch.float32)
    verify(got, ref, gl64, r, m, torch.float32, kind)
    if any(x.any() for x in m["out"].values()):
        moved, _ = run_temporal(out_moved(r, m), torch.float32)
        verify_moved(got, moved, r, torch.float32, _gv_bits(rb))
    _mark("fwd resident-window", rf)
    _mark("gather resident-window", rb)
    assert "owner-computes scatter kernel" in rb, rb          # the reader of the per-point records and their summaries


# ---- gradient subsets, the deterministic mode, windows with repeated frames -----------------------------------------------------
SUBSETS = [("value, per-point records", 1, {}), ("value, interval records", 1, {"MSDA_SCATTER_OWN": "0", "MSDA_BWD_CULL": "2"}),
           ("sampling", 2, {})]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,grads,env", SUBSETS, ids=[s[0] for s in SUBSETS])
def test_gradient_subsets(name, grads, env, kind, monkeypatch):
    _env(monkeypatch, env)
    d = temporal_case(195, _pyr(kind, [(12, 20), (6, 10), (3, 5)], [(16, 32), (8, 16), (4, 4)]), T=4, W=3, Lq=60)
    rf, rb = run_case(d, kind, 41, torch.float32, lambda r: run_temporal(r, torch.float32, grads=grads))
    _mark("value only (culling records)" if grads == 1 else "sampling only", rb)
    if grads == 1:
        assert ("owner-computes" in rb) == (not env), rb


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("det_route", ["1", "2"], ids=["any-shape", "lds-bands"])
def test_deterministic_grad_value_plain(det_route, kind, monkeypatch):
    """MSDA_GRAD_DETERMINISTIC (what torch.use_deterministic_algorithms(True) makes the autograd functions pass)."""
    monkeypatch.setenv("MSDA_DET_ROUTE", det_route)
    d = op_case(196, _pyr(kind, SMALL, POW2), N=2, M=8, D=32, Lq=60)
    rf, rb = run_case(d, kind, 43, torch.float32, lambda r: run_op(r, torch.float32, grads=7))
    assert "fixed-point" in rb and ("any shape" if det_route == "1" else "LDS bands") in rb, rb


@pytest.mark.parametrize("kind", CORE + ("piled",))
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_deterministic_grad_value_temporal_under_the_torch_flag(dtype, kind, monkeypatch):
    from devis_amd import _native
    from devis_amd.functions import MSDeformAttnTemporalFunction
    dt = DTYPES[dtype]
    ftab = np.array([[1, 1], [0, 2], [1, 0]], dtype=np.int32)
    d = temporal_case(197, _pyr(kind, [(12, 20), (6, 10), (3, 5)], [(16, 32), (8, 16), (4, 4)]), T=3, W=2, Lq=40, ftab=ftab)
    r, m = placed(d, kind, 45, dt)
    ref, gl64 = reference(r, dt)
    names = ("value", "loc_c", "aw_c", "loc_t", "aw_t")

    def fwd_bwd(x):
        ins = [_t(x[k], dt).requires_grad_(True) for k in names]
        out = MSDeformAttnTemporalFunction.apply(ins[0], _t(x["shapes"]), _t(x["lsi"]), _t(x["ftab"]), *ins[1:], 1)
        return (out,) + torch.autograd.grad(out, ins, _t(x["grad_out"], dt).view_as(out))
    routes, inner = [], _native.temporal_backward_grads      # (the backward runs on autograd's thread: its route is taken there)
    monkeypatch.setattr(_native, "temporal_backward_grads", lambda *a, **k: (inner(*a, **k), routes.append(_native.last_route()))[0])
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        got = fwd_bwd(r)
        moved = fwd_bwd(out_moved(r, m))
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    got, moved = ([_np(x.detach()) for x in y] for y in (got, moved))
    assert len(routes) == 2 and "fixed-point" in routes[0], routes
    verify(got, ref, gl64, r, m, dt, kind)
    verify_moved(got, moved, r, dt, "all")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_temporal_windows_with_repeated_frames(dtype, kind):
    ftab = np.array([[1, 1], [0, 2], [1, 3], [2, 4], [3, 3]], dtype=np.int32)
    dt = DTYPES[dtype]
    d = temporal_case(198, _pyr(kind, [(9, 7), (5, 4), (3, 2)], [(8, 8), (4, 4), (2, 2)]), T=5, W=2, Lq=45, Pt=2, ftab=ftab)
    rf, rb = run_case(d, kind, 49, dt, lambda r: run_temporal(r, dt))
    _mark("temporal, repeated frames", rb)


def test_every_route_was_reached():
    """Runs last: every route of test_layout_gpu.ROUTES showed up in msda_last_route() of a passing case of THIS file.  A case that
    did not run in this session (a -k selection) is not held against it."""
    missing = sorted(set(ROUTES) - SEEN)
    if len(SEEN) < 5:
        pytest.skip("the route cases of this file did not run in this session")
    assert not missing, missing
