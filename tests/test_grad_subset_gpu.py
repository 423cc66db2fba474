"""Backward of only the gradients autograd asks for (ABI v14: msda_backward_grads / msda_temporal_backward_grads, the
grads-mask Functions and ops).  GRAD_VALUE = grad_value, GRAD_SAMPLING = grad_sampling_loc + grad_attn_weight."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import PYR_A, make_inputs, make_temporal_inputs, oracle_fwd_bwd, temporal_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUE, SAMPLING, ALL = 1, 2, 3


@pytest.fixture(autouse=True)
def rules_only():
    """Route expectations are those of the rules: the shipped pins are taken out and put back afterwards."""
    from devis_amd import _native
    _native.load()
    _native.clear_routes()
    try:
        yield
    finally:
        _native.clear_routes()
        _native._load_shipped_routes()


def _dev(d, dtype=torch.float32, loc_dtype=None):
    out = {}
    for k, v in d.items():
        t = torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
        if t.is_floating_point():
            t = t.to(loc_dtype if (loc_dtype is not None and k.startswith(("loc", "aw"))) else dtype)
        out[k] = t
    return out


def _temporal(seed=0, T=3, Lq=40, shapes=((24, 40), (12, 20), (6, 10), (3, 5)), D=32, dtype=torch.float32, loc_dtype=None):
    d = make_temporal_inputs(seed, T=T, W=T - 1, M=8, D=D, Lq=Lq, shapes=list(shapes), Pc=4, Pt=4)
    return d, _dev(d, dtype, loc_dtype)


def _run_temporal(t, grads, value=None, workspace=None, storage_gv=False, clips=1):
    """One raw temporal backward call; returns (grad_value or None, [4 sampling grads] or None, route)."""
    from devis_amd import _native
    v = t["value"] if value is None else value
    L, Pc = t["loc_c"].shape[3], t["loc_c"].shape[4]
    gv = None
    if grads & VALUE:
        dt = _native.grad_value_dtype(v, t["shapes"], t["loc_c"].shape[1], L, Pc, clips=clips, window=t["ftab"].shape[1],
                                      Pt=t["loc_t"].shape[4]) if storage_gv else _native.acc_dtype(v.dtype)
        gv = torch.empty(v.shape, dtype=dt, device=DEV)
    gs = [torch.empty_like(t[k]) for k in ("loc_c", "aw_c", "loc_t", "aw_t")] if grads & SAMPLING else [None] * 4
    _native.temporal_backward_grads(grads, v, t["shapes"], t["lsi"], t["ftab"], t["loc_c"], t["aw_c"], t["loc_t"], t["aw_t"],
                                    t["grad_out"], clips, gv, *gs, workspace=workspace)
    torch.cuda.synchronize()
    return gv, (gs if grads & SAMPLING else None), _native.last_route()


def _nan_like(v):
    return torch.full_like(v, float("nan"))


# ---- 1. raw ABI -----------------------------------------------------------------------------------------------------

def test_abi_v14_symbols_zero_mask_null_outputs_and_untouched_sentinels():
    from devis_amd import _native
    lib = _native.load()
    assert lib.msda_version() == 14 and _native.MSDA_ABI_VERSION == 14
    from devis_amd import build
    raw = ctypes.CDLL(build.lib_path())
    assert hasattr(raw, "msda_backward_grads") and hasattr(raw, "msda_temporal_backward_grads")
    d, t = _temporal()
    # grads = 0: nothing launched, nothing written
    gv = torch.full(t["value"].shape, 7.0, device=DEV)
    gs = [torch.full_like(t[k], 7.0) for k in ("loc_c", "aw_c", "loc_t", "aw_t")]
    _native.temporal_backward_grads(0, t["value"], t["shapes"], t["lsi"], t["ftab"], t["loc_c"], t["aw_c"], t["loc_t"],
                                    t["aw_t"], t["grad_out"], 1, gv, *gs)
    torch.cuda.synchronize()
    assert _native.last_route() == ""
    assert bool((gv == 7).all()) and all(bool((g == 7).all()) for g in gs)
    # bits outside the two groups: an argument error
    with pytest.raises(RuntimeError, match="grads"):
        _native.temporal_backward_grads(4, t["value"], t["shapes"], t["lsi"], t["ftab"], t["loc_c"], t["aw_c"], t["loc_t"],
                                        t["aw_t"], t["grad_out"], 1, gv, *gs)
    # NULL outputs for the group not asked for, and sentinels passed there come back untouched
    full_v, full_s, _ = _run_temporal(t, ALL)
    v_only, _, _ = _run_temporal(t, VALUE)                       # (sampling outputs NULL)
    _, s_only, _ = _run_temporal(t, SAMPLING)                    # (grad_value NULL, no workspace)
    assert torch.isfinite(v_only).all()
    for a, b in zip(s_only, full_s):
        assert torch.equal(a, b)
    sentinel_s = [torch.full_like(t[k], 7.0) for k in ("loc_c", "aw_c", "loc_t", "aw_t")]
    _native.temporal_backward_grads(VALUE, t["value"], t["shapes"], t["lsi"], t["ftab"], t["loc_c"], t["aw_c"], t["loc_t"],
                                    t["aw_t"], t["grad_out"], 1, torch.empty_like(full_v), *sentinel_s)
    sentinel_v = torch.full(t["value"].shape, 7.0, device=DEV)
    _native.temporal_backward_grads(SAMPLING, t["value"], t["shapes"], t["lsi"], t["ftab"], t["loc_c"], t["aw_c"],
                                    t["loc_t"], t["aw_t"], t["grad_out"], 1, sentinel_v, *[torch.empty_like(g) for g in full_s])
    torch.cuda.synchronize()
    assert all(bool((g == 7).all()) for g in sentinel_s) and bool((sentinel_v == 7).all())


# ---- 2. GRAD_VALUE never reads value ---------------------------------------------------------------------------------

ROUTES = {
    "owner_mfma": {"MSDA_SCATTER_MFMA": "1"},
    "owner_no_mfma": {"MSDA_SCATTER_MFMA": "0"},
    "lds_atomic_intervals": {"MSDA_SCATTER_OWN": "0", "MSDA_BWD_CULL": "2"},
    "lds_atomic_points": {"MSDA_SCATTER_OWN": "0"},
    "generic": {"MSDA_FORCE_GENERIC": "1"},
}


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("dtype,loc_dtype", [(torch.float32, None), (torch.bfloat16, None), (torch.float16, None),
                                             (torch.bfloat16, torch.float32)], ids=["f32", "bf16", "f16", "bf16_loc32"])
def test_value_group_ignores_value_and_matches_full_call_and_oracle(monkeypatch, route, dtype, loc_dtype):
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    d, t = _temporal(seed=1, dtype=dtype, loc_dtype=loc_dtype)
    full, _, full_route = _run_temporal(t, ALL)
    got, _, r = _run_temporal(t, VALUE, value=_nan_like(t["value"]))
    assert torch.isfinite(got).all()
    assert "grad_loc/grad_attn" not in r, r
    if route != "generic":
        assert "culling records" in r and "scatter" in r.lower(), r
    else:
        assert "grad_value only" in r, r
    if route.startswith("lds_atomic"):
        assert torch.equal(got, full)                        # the fp64 LDS scatter is order independent
    else:
        assert float((got - full).abs().max()) <= 2e-6 * float(full.abs().max())      # run-to-run spread of float sums
    ref = temporal_reference(*(t[k].double().cpu().numpy() if t[k].is_floating_point() else t[k].cpu().numpy()
                               for k in ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out")))
    tol = 1e-4 if dtype == torch.float32 else 1e-2
    assert float(np.abs(got.double().cpu().numpy() - ref[1]).max()) <= tol * max(1.0, float(np.abs(ref[1]).max()))


def test_value_group_storage_typed_grad_value_and_plain_entry_with_im2col_chunks():
    from devis_amd import _native
    from devis_amd.functions import ms_deform_attn_func as F
    # storage-typed (bf16) grad_value on the owner-computes scatter
    d, t = _temporal(seed=2, dtype=torch.bfloat16)
    full, _, _ = _run_temporal(t, ALL, storage_gv=True)
    assert full.dtype == torch.bfloat16
    got, _, r = _run_temporal(t, VALUE, value=_nan_like(t["value"]), storage_gv=True)
    assert "culling records" in r
    assert float((got.float() - full.float()).abs().max()) <= 2 * float(full.float().abs().max()) * 2 ** -8
    # plain entry point, im2col_step 2 over a batch of 4
    p = make_inputs(3, N=4, M=8, D=32, Lq=50, shapes=PYR_A[1:], P=4)
    tp = _dev(p)
    gv_full, gl_full, ga_full = F._backward(tp["value"], tp["shapes"], tp["lsi"], tp["loc"], tp["aw"], tp["grad_out"], 2)
    gv, gl, ga = F._backward(_nan_like(tp["value"]), tp["shapes"], tp["lsi"], tp["loc"], tp["aw"], tp["grad_out"], 2,
                             grads=VALUE)
    assert gl is None and ga is None and "culling records" in _native.last_route()
    assert float((gv - gv_full).abs().max()) <= 2e-6 * float(gv_full.abs().max())
    _, ref_gv, _, _ = oracle_fwd_bwd(p)
    assert float(np.abs(gv.double().cpu().numpy() - ref_gv).max()) <= 1e-4 * max(1.0, float(np.abs(ref_gv).max()))
    gv2, gl2, ga2 = F._backward(tp["value"], tp["shapes"], tp["lsi"], tp["loc"], tp["aw"], tp["grad_out"], 2, grads=SAMPLING)
    assert gv2 is None and torch.equal(gl2, gl_full) and torch.equal(ga2, ga_full)


def test_value_and_sampling_groups_on_the_one_kernel_tile_route():
    """9 frames with 8 temporal slots: 73 sources per pixel exceed the scatter's lists -> the one-kernel tile backward."""
    d, t = _temporal(seed=4, T=9, Lq=20, shapes=((12, 20), (6, 10)))
    full, full_s, full_route = _run_temporal(t, ALL)
    assert "tile kernel, global atomics" in full_route, full_route
    got, _, r = _run_temporal(t, VALUE, value=_nan_like(t["value"]))
    assert "tile kernel, grad_value only" in r and "culling" not in r, r
    assert float((got - full).abs().max()) <= 2e-6 * float(full.abs().max())
    _, s_only, r = _run_temporal(t, SAMPLING)
    assert "tile kernel, grad_loc/grad_attn" in r and "atomics" not in r, r
    for a, b in zip(s_only, full_s):
        assert torch.equal(a, b)


def test_value_and_sampling_groups_in_f64():
    from devis_amd.functions import ms_deform_attn_func as F
    from devis_amd import _native
    p = make_inputs(4, N=2, M=4, D=24, Lq=30, shapes=PYR_A[2:], P=4)
    tp = _dev(p, torch.float64)
    gv_full, gl_full, ga_full = F._backward(tp["value"], tp["shapes"], tp["lsi"], tp["loc"], tp["aw"], tp["grad_out"], 1)
    gv, gl, ga = F._backward(_nan_like(tp["value"]), tp["shapes"], tp["lsi"], tp["loc"], tp["aw"], tp["grad_out"], 1,
                             grads=VALUE)
    assert "generic kernel, grad_value only" in _native.last_route() and gl is None and ga is None
    assert float((gv - gv_full).abs().max()) <= 1e-12 * float(gv_full.abs().max())
    _, ref_gv, _, _ = oracle_fwd_bwd(p)
    assert float(np.abs(gv.cpu().numpy() - ref_gv).max()) <= 1e-10 * max(1.0, float(np.abs(ref_gv).max()))
    gv, gl, ga = F._backward(tp["value"], tp["shapes"], tp["lsi"], tp["loc"], tp["aw"], tp["grad_out"], 1, grads=SAMPLING)
    r = _native.last_route()
    assert gv is None and "atomics" not in r and "generic kernel, grad_loc/grad_attn" in r, r
    assert torch.equal(gl, gl_full) and torch.equal(ga, ga_full)


# ---- 3. GRAD_SAMPLING is bitwise the full call's -----------------------------------------------------------------------

GATHER = {
    "win": ({"MSDA_BWD_WIN": "1"}, None, "resident-window"),
    "rs": ({"MSDA_BWD_RS": "1", "MSDA_BWD_RS_FSPLIT": "0", "MSDA_BWD_WIN": "0"}, 40, "resident-slab"),
    "rs_fsplit": ({"MSDA_BWD_RS": "1", "MSDA_BWD_RS_FSPLIT": "2", "MSDA_BWD_WIN": "0"}, 40, "one source frame"),
    "tile": ({"MSDA_BWD_RS": "0", "MSDA_BWD_WIN": "0"}, 40, "tile kernel"),
    "generic": ({"MSDA_FORCE_GENERIC": "1"}, 40, "generic kernel"),
}


@pytest.mark.parametrize("route", sorted(GATHER))
def test_sampling_group_is_bitwise_the_full_calls_and_launches_no_scatter(monkeypatch, route):
    env, Lq, name = GATHER[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    shapes = ((24, 40), (12, 20), (6, 10), (3, 5))
    if Lq is None:
        Lq = sum(h * w for h, w in shapes)          # encoder-shaped: one query per pixel
    d, t = _temporal(seed=5, T=3, Lq=Lq, shapes=shapes)
    _, full_s, full_route = _run_temporal(t, ALL)
    _, got, r = _run_temporal(t, SAMPLING)
    assert name in r and name in full_route, (r, full_route)
    if route != "generic":                                          # (generic: a kernel of its own, see msda_generic.hip)
        assert r == full_route.split("; ")[0], (r, full_route)      # the full call's gather kernel, nothing after it
    assert "scatter" not in r.lower() and "zero-fill" not in r and "culling" not in r, r
    for a, b in zip(got, full_s):
        assert torch.equal(a, b)


# No gather route forced: the gather kernel follows from the records the full call's scatter reads.  Interval records
# (LDS-atomic scatter: MSDA_SCATTER_OWN=0, MSDA_BWD_CULL=2, or more than 4 points per level) are written by the tile kernel
# only, so the full call's gather pass runs there -- and a GRAD_SAMPLING call, which passes no workspace, must run it too.
@pytest.mark.parametrize("case", ["scatter_own_0", "bwd_cull_2", "points_8", "owner_default", "encoder_default"])
def test_sampling_group_takes_the_full_calls_gather_kernel_without_a_workspace(monkeypatch, case):
    env = {"scatter_own_0": {"MSDA_SCATTER_OWN": "0"}, "bwd_cull_2": {"MSDA_BWD_CULL": "2"}}.get(case, {})
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    P = 8 if case == "points_8" else 4
    shapes = ((24, 40), (12, 20), (6, 10), (3, 5))
    Lq = sum(h * w for h, w in shapes) if case == "encoder_default" else 40
    d = make_temporal_inputs(8, T=3, W=2, M=8, D=32, Lq=Lq, shapes=list(shapes), Pc=P, Pt=P)
    t = _dev(d)
    _, full_s, full_route = _run_temporal(t, ALL)
    _, got, r = _run_temporal(t, SAMPLING)
    if case in ("scatter_own_0", "bwd_cull_2", "points_8"):
        assert "tile kernel, grad_loc/grad_attn" in full_route, full_route
    assert r == full_route.split("; ")[0], (r, full_route)
    for a, b in zip(got, full_s):
        assert torch.equal(a, b)


# ---- 4. the records a GRAD_VALUE call leaves are the gather pass's ---------------------------------------------------

@pytest.mark.parametrize("form", ["points", "intervals"])
@pytest.mark.parametrize("shape", ["cfg3_2clips", "encoder_1clip"])
def test_value_group_records_are_byte_identical(monkeypatch, form, shape):
    from devis_amd import _native
    if form == "intervals":
        monkeypatch.setenv("MSDA_SCATTER_OWN", "0")
        monkeypatch.setenv("MSDA_BWD_CULL", "2")
    monkeypatch.setenv("MSDA_SCATTER_MFMA", "0")
    clips, T = (2, 3) if shape == "cfg3_2clips" else (1, 3)
    shapes = PYR_A
    Lq = 60 if shape == "cfg3_2clips" else sum(h * w for h, w in shapes)
    d = make_temporal_inputs(6, T=T, W=T - 1, M=8, D=32, Lq=Lq, shapes=shapes, Pc=4, Pt=4)
    t = _dev({k: (np.concatenate([v] * clips) if k in ("value", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out") else v)
              for k, v in d.items()})
    G, M, L, W = clips * T, 8, len(shapes), T - 1
    n = _native.load().msda_backward_workspace_bytes(G, Lq, M, L * (1 + W))
    ws_full = torch.full(((n + 3) // 4,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    ws_val = ws_full.clone()
    _native.temporal_backward(t["value"], t["shapes"], t["lsi"], t["ftab"], t["loc_c"], t["aw_c"], t["loc_t"], t["aw_t"],
                              t["grad_out"], clips, torch.empty(t["value"].shape, device=DEV),
                              *[torch.empty_like(t[k]) for k in ("loc_c", "aw_c", "loc_t", "aw_t")], workspace=ws_full)
    _run_temporal(t, VALUE, value=_nan_like(t["value"]), workspace=ws_val, clips=clips)
    a, b = ws_full.cpu().numpy(), ws_val.cpu().numpy()
    # the ticket counters: zeroed by the records kernel as by the gather pass, then drawn down alike by the same scatter
    assert (a[:16] != 0x5A5A5A5A).all() and (a[:16] == b[:16]).all()
    if form == "intervals":
        assert (a == b).all()
        return
    # per-point records: the levels the owner-computes scatter reads (more than one band: > 1024 pixels) are written by
    # both calls byte for byte; the gather pass may also leave records of other levels, the records kernel does not
    rec = lambda w: w[16:16 + G * M * L * (1 + W) * Lq * 2].reshape(G, M, L * (1 + W), Lq, 2)     # noqa: E731
    ra, rb = rec(a), rec(b)
    for vl in range(L * (1 + W)):
        h, w = shapes[vl % L]
        if h * w > 1024:
            assert (ra[:, :, vl] == rb[:, :, vl]).all(), vl
            assert (rb[:, :, vl] != 0x5A5A5A5A).any()
        else:
            assert (rb[:, :, vl] == 0x5A5A5A5A).all(), vl
    written = b != 0x5A5A5A5A
    assert (a[written] == b[written]).all()                            # block summaries included


# ---- 5. autograd --------------------------------------------------------------------------------------------------

SUBSETS = [(v, l, a) for v in (0, 1) for l in (0, 1) for a in (0, 1) if v or l or a]


@pytest.mark.parametrize("D", [30, 32, 64])
@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "v%dl%da%d" % s)
def test_gradcheck_every_requires_grad_subset(monkeypatch, D, subset):
    """The reference's check_gradient_numerical(channels, grad_value, grad_sampling_loc, grad_attn_weight) (test.py:60-72)."""
    from devis_amd import _native
    from devis_amd.functions import MSDeformAttnFunction
    seen = []
    orig_grads = _native.backward_grads
    monkeypatch.setattr(_native, "backward_grads", lambda g, *a, **k: (seen.append(g), orig_grads(g, *a, **k))[1])
    p = make_inputs(7, N=1, M=2, D=D, Lq=2, shapes=[(6, 4), (3, 2)], P=2, loc_mode="unit")
    t = _dev(p, torch.float64)
    value = t["value"].requires_grad_(bool(subset[0]))
    loc = t["loc"].requires_grad_(bool(subset[1]))
    aw = t["aw"].requires_grad_(bool(subset[2]))
    fn = lambda v, l, a: MSDeformAttnFunction.apply(v, t["shapes"], t["lsi"], l, a, 1)     # noqa: E731
    assert torch.autograd.gradcheck(fn, (value, loc, aw), eps=1e-6, atol=1e-4, rtol=1e-2)
    want = (VALUE if subset[0] else 0) | (SAMPLING if subset[1] or subset[2] else 0)
    assert seen and set(seen) == {want}
    out = fn(value, loc, aw)
    got = out.grad_fn.apply(torch.ones_like(out))          # the Function's own gradient slots: None where skipped
    for g, s in zip((got[0], got[3], got[4]), subset):
        assert (g is not None) == bool(s)


# ---- 6. modules ---------------------------------------------------------------------------------------------------

def _decoder(freeze):
    from module_cases import cfg_build
    from devis_amd.modules import TemporalMSDeformAttnDecoder
    mod, args, loss_w = cfg_build("dec", TemporalMSDeformAttnDecoder, torch.float32)
    mod = mod.to(DEV)
    mv = lambda x: x.to(DEV) if isinstance(x, torch.Tensor) else type(x)(y.to(DEV) for y in x)     # noqa: E731
    args = [mv(a) for a in args]
    for k, p in mod.named_parameters():
        if any(f in k for f in freeze):
            p.requires_grad_(False)
    return mod, args, loss_w.to(DEV)


def _param_grads(mod, args, loss_w, query_grad, input_grad):
    args = list(args)
    args[0] = args[0].detach().requires_grad_(query_grad)
    args[2] = args[2].detach().requires_grad_(input_grad)
    out = mod(*args)[0]
    names = [k for k, p in sorted(mod.named_parameters()) if p.requires_grad]
    gs = torch.autograd.grad((out * loss_w).sum(), [dict(mod.named_parameters())[k] for k in names])
    return dict(zip(names, gs))


def test_decoder_with_frozen_value_proj_runs_the_sampling_path_bitwise(monkeypatch):
    from devis_amd import _native
    seen = []
    orig = _native.temporal_backward_grads
    monkeypatch.setattr(_native, "temporal_backward_grads", lambda g, *a, **k: (seen.append(g), orig(g, *a, **k))[1])
    mod, args, loss_w = _decoder(())
    full = _param_grads(mod, args, loss_w, True, True)
    for k, p in mod.named_parameters():
        if "value_proj" in k:
            p.requires_grad_(False)
    part = _param_grads(mod, args, loss_w, True, False)
    assert seen == [ALL, SAMPLING]                                # the full backward, then the partial one
    assert part and all(torch.equal(part[k], full[k]) for k in part), [k for k in part if not torch.equal(part[k], full[k])]


def test_decoder_with_frozen_sampling_side_runs_the_value_path(monkeypatch):
    from devis_amd import _native
    seen = []
    orig = _native.temporal_backward_grads
    monkeypatch.setattr(_native, "temporal_backward_grads", lambda g, *a, **k: (seen.append(g), orig(g, *a, **k))[1])
    mod, args, loss_w = _decoder(())
    full = _param_grads(mod, args, loss_w, True, True)
    for k, p in mod.named_parameters():
        if "value_proj" not in k:
            p.requires_grad_(False)
    part = _param_grads(mod, args, loss_w, False, True)
    assert seen == [ALL, VALUE]                                   # the full backward, then the partial one
    assert set(part) == {k for k in full if "value_proj" in k}
    for k in part:
        assert float((part[k] - full[k]).abs().max()) <= 1e-5 * max(1.0, float(full[k].abs().max())), k


def test_msdeformattn_compiled_with_frozen_value_proj_matches_eager():
    from devis_amd.modules import MSDeformAttn
    torch.manual_seed(0)
    shapes = torch.tensor(PYR_A[1:], dtype=torch.int64, device=DEV)
    lsi = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    S = int(shapes.prod(1).sum())
    mod = MSDeformAttn(d_model=256, n_levels=3, n_heads=8, n_points=4).to(DEV)
    mod.value_proj.requires_grad_(False)
    query = torch.randn(2, 50, 256, device=DEV)
    ref = torch.rand(2, 50, 3, 2, device=DEV)
    src = torch.randn(2, S, 256, device=DEV)

    def grads(m):
        out = m(query, ref, src, shapes, lsi, None)[0]
        ps = [p for _, p in sorted(mod.named_parameters()) if p.requires_grad]
        return torch.autograd.grad(out.square().sum(), ps)

    eager = grads(mod)
    compiled = torch.compile(mod, fullgraph=True)
    got = grads(compiled)
    for a, b in zip(got, eager):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def test_graphed_layer_with_frozen_value_proj_replays_the_partial_backward(monkeypatch):
    from devis_amd import _native, graph_stream, graphed
    from devis_amd.modules import MSDeformAttn
    torch.manual_seed(1)
    shapes = torch.tensor(PYR_A[1:], dtype=torch.int64, device=DEV)
    lsi = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    S = int(shapes.prod(1).sum())
    mod = MSDeformAttn(d_model=256, n_levels=3, n_heads=8, n_points=4).to(DEV)
    mod.value_proj.requires_grad_(False)
    query = torch.randn(1, 40, 256, device=DEV)
    ref = torch.rand(1, 40, 3, 2, device=DEV)
    src = torch.randn(1, S, 256, device=DEV)
    ps = [p for _, p in sorted(mod.named_parameters()) if p.requires_grad]
    eager = torch.autograd.grad(mod(query, ref, src, shapes, lsi, None)[0].square().sum(), ps)
    seen = []
    part = _native.backward_grads
    monkeypatch.setattr(_native, "backward_grads", lambda g, *a, **k: (seen.append(g), part(g, *a, **k))[1])
    layer = graphed(mod)
    with graph_stream():
        for _ in range(3):
            got = torch.autograd.grad(layer(query, ref, src, shapes, lsi, None)[0].square().sum(), ps)
    torch.cuda.synchronize()
    assert layer.eager_calls == 0 and layer.graphs >= 1          # captured and replayed, not run eagerly
    assert seen and set(seen) == {SAMPLING}                      # the captured backward is the partial one
    for a, b in zip(got, eager):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
