"""GPU parity tests of the operator: HIP kernels (through the C ABI, via the reference-shaped
autograd.Function) against the CPU oracle and the committed golden vectors.

Tolerances: BASELINE.json asks <= 1e-4 max-abs in fp32 and <= 1e-2 in bf16 vs the reference oracle on
identical (already rounded) inputs; the bounds used here are much tighter and written per test."""
import os

import numpy as np
import pytest
import torch

from conftest import OP_FIXTURES, golden
from devis_amd.tuning import kSdbgNoBandRotation, kSdbgNoFourSlotRule, kSdbgSeparateZero, kSdbgStaticStride
from helpers import (PYR_A, localise, make_inputs, make_temporal_inputs, oracle_fwd_bwd, round_to,
                     temporal_reference)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STATIC = str(kSdbgStaticStride)        # MSDA_SCATTER_DBG: static item stride


def _run_op(d, dtype, step=64):
    from devis_amd.functions import MSDeformAttnFunction
    v, l, a = (torch.from_numpy(np.asarray(d[k], dtype=np.float64)).to(DEV, dtype).requires_grad_(True)
               for k in ("value", "loc", "aw"))
    shapes = torch.from_numpy(d["shapes"]).to(DEV)
    lsi = torch.from_numpy(d["lsi"]).to(DEV)
    out = MSDeformAttnFunction.apply(v, shapes, lsi, l, a, step)
    go = torch.from_numpy(np.asarray(d["grad_out"], dtype=np.float64)).to(DEV, dtype)
    gv, gl, ga = torch.autograd.grad(out, (v, l, a), go)
    torch.cuda.synchronize()
    return [t.detach().double().cpu().numpy() for t in (out, gv, gl, ga)]


def _direct_temporal_backward_route(value, shapes, lsi, ftab, loc_c, aw_c, loc_t, aw_t, grad_out, clips):
    """msda_last_route() of the backward of a fused temporal call (the route string is per thread, and autograd runs the
    backward on a thread of its own: the call is repeated here, on this thread, with buffers as the autograd function
    allocates them)."""
    from devis_amd import _native
    t = [x.detach() for x in (value, loc_c, aw_c, loc_t, aw_t)]
    L, P, W = loc_c.shape[3], loc_c.shape[4], ftab.shape[1]
    gv = torch.empty(value.shape, device=value.device,
                     dtype=_native.grad_value_dtype(t[0], shapes, loc_c.shape[1], L, P, clips=clips, window=W, Pt=loc_t.shape[4]))
    grads = [torch.empty_like(x) for x in t[1:]]
    _native.temporal_backward(t[0], shapes, lsi, ftab, t[1], t[2], t[3], t[4], grad_out, clips, gv, *grads)
    torch.cuda.synchronize()
    return _native.last_route()


def _golden_dict(name):
    g = golden(name)
    return g, dict(value=g["value"], shapes=g["spatial_shapes"], lsi=g["level_start_index"],
                   loc=g["sampling_locations"], aw=g["attention_weights"], grad_out=g["grad_output"])


def _maxabs(a, b):
    return float(np.abs(a - b).max()) if a.size else 0.0


@pytest.mark.parametrize("name", OP_FIXTURES)
def test_fp64_matches_golden(name):
    """Reference test.py:30-42 (fp64 forward allclose) + gradients, on every golden fixture."""
    g, d = _golden_dict(name)
    out, gv, gl, ga = _run_op(d, torch.float64)
    np.testing.assert_allclose(out, g["out"], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(gv, g["grad_value"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(ga, g["grad_attn_weight"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(gl, g["grad_sampling_loc"], rtol=1e-8, atol=1e-11)


@pytest.mark.parametrize("name", OP_FIXTURES)
def test_fp32_matches_golden(name):
    g, d = _golden_dict(name)
    out, gv, gl, ga = _run_op(d, torch.float32)
    assert _maxabs(out, g["out"]) <= 1e-6          # BASELINE bar: 1e-4
    scale = lambda x: max(1.0, float(np.abs(x).max()))
    assert _maxabs(gv, g["grad_value"]) <= 2e-5 * scale(g["grad_value"])
    assert _maxabs(ga, g["grad_attn_weight"]) <= 2e-5 * scale(g["grad_attn_weight"])
    assert _maxabs(gl, g["grad_sampling_loc"]) <= 2e-5 * scale(g["grad_sampling_loc"])


@pytest.mark.parametrize("name", ["op_devis_small", "op_cfg1", "op_generic_D64", "op_out_of_range"])
def test_generic_kernels_fp32(name, monkeypatch):
    """MSDA_FORCE_GENERIC=1 routes fp32 through the any-shape kernels."""
    monkeypatch.setenv("MSDA_FORCE_GENERIC", "1")
    g, d = _golden_dict(name)
    out, gv, gl, ga = _run_op(d, torch.float32)
    assert _maxabs(out, g["out"]) <= 1e-6
    assert _maxabs(gv, g["grad_value"]) <= 2e-5 * max(1.0, np.abs(g["grad_value"]).max())
    assert _maxabs(gl, g["grad_sampling_loc"]) <= 2e-5 * max(1.0, np.abs(g["grad_sampling_loc"]).max())
    assert _maxabs(ga, g["grad_attn_weight"]) <= 2e-5 * max(1.0, np.abs(g["grad_attn_weight"]).max())


@pytest.mark.parametrize("slab", ["auto", "forced"])
@pytest.mark.parametrize("dtype,tol_out,tol_rel", [(torch.bfloat16, 1e-2, 2e-2), (torch.float16, 1e-3, 4e-3)])
@pytest.mark.parametrize("D", [32, 64, 8])
def test_reduced_precision_vs_fp64_oracle_on_rounded_inputs(dtype, tol_out, tol_rel, D, slab, monkeypatch):
    """bf16/f16 storage, fp32 arithmetic.  The oracle runs in fp64 on the SAME rounded inputs.
    `forced`: the resident-slab kernels where they apply (D = 32), which this small shape would not pick."""
    if slab == "forced":
        monkeypatch.setenv("MSDA_FWD_RS", "1"); monkeypatch.setenv("MSDA_BWD_RS", "1")
    d = make_inputs(7, 2, 8, D, 33, [(12, 20), (6, 10), (3, 5), (2, 3)], 4, "wide", np.float64, value_scale=1.0)
    d = round_to(d, dtype)
    ref = oracle_fwd_bwd(d, np.float64)
    got = _run_op(d, dtype)
    assert _maxabs(got[0], ref[0]) <= tol_out * max(1.0, np.abs(ref[0]).max())
    for a, b in zip(got[1:], ref[1:]):
        assert _maxabs(a, b) <= tol_rel * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("step", [1, 2, 3, 6, 64])
def test_im2col_step_is_result_neutral(step):
    """ms_deform_attn_cuda.cu:50-75: chunked launches with pointer offsets."""
    g, d = _golden_dict("op_batched_im2col")
    out, gv, gl, ga = _run_op(d, torch.float64, step=step)
    np.testing.assert_allclose(out, g["out"], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(gv, g["grad_value"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(gl, g["grad_sampling_loc"], rtol=1e-8, atol=1e-11)


def test_im2col_step_must_divide_batch():
    """cu:52: batch % min(batch, im2col_step) != 0 raises."""
    from devis_amd.functions import MSDeformAttnFunction
    _, d = _golden_dict("op_batched_im2col")      # N = 6
    args = [torch.from_numpy(d[k]).to(DEV) for k in ("value", "shapes", "lsi", "loc", "aw")]
    with pytest.raises(RuntimeError, match="must divide"):
        MSDeformAttnFunction.apply(*args, 4)


def test_error_contract():
    from devis_amd.functions import MSDeformAttnFunction
    _, d = _golden_dict("op_testpy_shape")
    v, s, i, l, a = [torch.from_numpy(d[k]) for k in ("value", "shapes", "lsi", "loc", "aw")]
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):       # ms_deform_attn.h:38
        MSDeformAttnFunction.apply(v, s, i, l, a, 2)
    v, s, i, l, a = [t.to(DEV) for t in (v, s, i, l, a)]
    with pytest.raises(RuntimeError, match="contiguous"):                       # cu:28-32
        MSDeformAttnFunction.apply(v.transpose(2, 3).contiguous().transpose(2, 3), s, i, l, a, 2)
    with pytest.raises(RuntimeError):
        MSDeformAttnFunction.apply(v, s, i, l.double(), a, 2)


def test_gradcheck_fp64_reference_procedure():
    """Reference test.py:61-84: gradcheck at D in {30,32,64,71,1025} on its shapes (2048/3096 only
    repeat the D>1024 kernel classes of the reference and are skipped for time)."""
    from devis_amd.functions import MSDeformAttnFunction
    N, M, Lq, L, P = 1, 2, 2, 2, 2
    shapes = torch.as_tensor([(6, 4), (3, 2)], dtype=torch.long, device=DEV)
    lsi = torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
    S = 30
    torch.manual_seed(3)
    for D in (30, 32, 64, 71, 1025):
        value = (torch.rand(N, S, M, D, device=DEV) * 0.01).double().requires_grad_(True)
        loc = torch.rand(N, Lq, M, L, P, 2, device=DEV).double().requires_grad_(True)
        aw = torch.rand(N, Lq, M, L, P, device=DEV) + 1e-5
        aw = (aw / aw.sum(-1, keepdim=True).sum(-2, keepdim=True)).double().requires_grad_(True)
        assert torch.autograd.gradcheck(MSDeformAttnFunction.apply, (value, shapes, lsi, loc, aw, 2))


def test_tail_tile_and_empty():
    """Query counts that do not fill a wave tile, and empty inputs."""
    from devis_amd.functions import MSDeformAttnFunction
    for Lq in (1, 7, 9, 65):
        d = make_inputs(100 + Lq, 2, 8, 32, Lq, [(5, 7), (3, 4)], 3, "wide", np.float32)
        ref = oracle_fwd_bwd(d, np.float64)
        got = _run_op(d, torch.float32)
        assert _maxabs(got[0], ref[0]) <= 1e-6
        assert _maxabs(got[1], ref[1]) <= 1e-4 and _maxabs(got[2], ref[2]) <= 1e-3 and _maxabs(got[3], ref[3]) <= 1e-4
    d = make_inputs(1, 1, 8, 32, 1, [(5, 7)], 2)
    v, s, i = (torch.from_numpy(d[k]).to(DEV) for k in ("value", "shapes", "lsi"))
    out = MSDeformAttnFunction.apply(v, s, i, torch.zeros(1, 0, 8, 1, 2, 2, device=DEV),
                                     torch.zeros(1, 0, 8, 1, 2, device=DEV), 64)
    assert out.shape == (1, 0, 256)


def test_devis_decoder_call_shapes_fp32():
    """cfg3 per-frame calls at full size: current (L=4) and temporal (L=20, S_in=5S), 300 queries."""
    for L_rep, seed in ((1, 5), (5, 6)):
        d = make_inputs(seed, 1, 8, 32, 300, PYR_A * L_rep, 4, "wide", np.float32)
        ref64 = oracle_fwd_bwd(d, np.float64)
        # grad_loc is discontinuous where a pixel coordinate crosses an integer, so a point within one
        # fp32 ulp of a cell border may legitimately land in the other cell than in fp64 arithmetic:
        # gradients are compared with the oracle evaluated in the SAME (fp32) arithmetic, whose
        # x*W-0.5 rounding the kernel reproduces bit for bit; the output (continuous) also vs fp64.
        ref32 = oracle_fwd_bwd(d, np.float32)
        got = _run_op(d, torch.float32)
        assert _maxabs(got[0], ref64[0]) <= 1e-6
        assert _maxabs(got[1], ref32[1]) <= 1e-4
        assert _maxabs(got[2], ref32[2]) <= 1e-4 * max(1.0, np.abs(ref32[2]).max())
        assert _maxabs(got[3], ref32[3]) <= 1e-4


# ---------------------------------------------------------------------------------------------
# fused temporal op
# ---------------------------------------------------------------------------------------------
def _run_temporal(d, dtype, clips=1, head_major=False):
    from devis_amd import _native
    from devis_amd.functions import MSDeformAttnTemporalFunction
    f = lambda k: torch.from_numpy(np.asarray(d[k], dtype=np.float64)).to(DEV, dtype).requires_grad_(True)
    v, lc, ac, lt, at = f("value"), f("loc_c"), f("aw_c"), f("loc_t"), f("aw_t")
    if head_major:
        v = _native.head_major(v.detach()).requires_grad_(True)
    shapes = torch.from_numpy(d["shapes"]).to(DEV)
    lsi = torch.from_numpy(d["lsi"]).to(DEV)
    ftab = torch.from_numpy(d["ftab"]).to(DEV)
    out = MSDeformAttnTemporalFunction.apply(v, shapes, lsi, ftab, lc, ac, lt, at, clips)
    go = torch.from_numpy(np.asarray(d["grad_out"], dtype=np.float64)).to(DEV, dtype)
    grads = torch.autograd.grad(out, (v, lc, ac, lt, at), go)
    torch.cuda.synchronize()
    return [t.detach().double().cpu().numpy() for t in (out,) + tuple(grads)]


@pytest.mark.parametrize("dtype,D", [(torch.float64, 32), (torch.float32, 32), (torch.float32, 20),
                                     (torch.float64, 7)])
def test_temporal_fused_equals_reference_call_pattern(dtype, D):
    d = make_temporal_inputs(21, T=4, W=3, M=8, D=D, Lq=19, shapes=[(6, 5), (3, 3)], Pc=4, Pt=2)
    ref = temporal_reference(*(np.asarray(d[k], dtype=np.float64) if d[k].dtype.kind == "f" else d[k]
                               for k in ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t",
                                         "grad_out")))
    got = _run_temporal(d, dtype)
    tol = 1e-11 if dtype == torch.float64 else 2e-5
    for a, b in zip(got, ref):
        assert _maxabs(a, b) <= tol * max(1.0, np.abs(b).max())


def test_temporal_fused_window_with_repeated_frames_and_clips():
    """Mirrored window (devis_transformer.py:103-113: repeated frame ids) and a batch of clips."""
    T, W = 5, 2
    ftab = np.array([[1, 1], [0, 2], [1, 3], [2, 4], [3, 3]], dtype=np.int32)
    clips = 3
    ds = [make_temporal_inputs(30 + c, T, W, 8, 32, 11, [(6, 5), (3, 3)], 3, 2, ftab=ftab) for c in range(clips)]
    cat = {k: (np.concatenate([x[k] for x in ds], 0) if k not in ("shapes", "lsi", "ftab") else ds[0][k])
           for k in ds[0]}
    got = _run_temporal(cat, torch.float32, clips=clips)
    for c, d in enumerate(ds):
        ref = temporal_reference(*(np.asarray(d[k], dtype=np.float64) if d[k].dtype.kind == "f" else d[k]
                                   for k in ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t",
                                             "grad_out")))
        for a, b in zip(got, ref):
            assert _maxabs(a[c * T:(c + 1) * T], b) <= 2e-5 * max(1.0, np.abs(b).max())


def test_full_size_properties_cfg3():
    """BASELINE cfg3 at full size (T=6, q=300, pyramid A, L=4, K=4, C=256), through size-independent
    properties: linearity in value, the sum rule for constant value maps, and fwd/bwd adjointness."""
    from devis_amd.functions import MSDeformAttnTemporalFunction
    d = make_temporal_inputs(77, T=6, W=5, M=8, D=32, Lq=300, shapes=PYR_A, Pc=4, Pt=4)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}
    # in-range locations only for the constant-map rule
    run = lambda v, lc, lt: MSDeformAttnTemporalFunction.apply(
        v, t["shapes"], t["lsi"], t["ftab"], lc, t["aw_c"], lt, t["aw_t"], 1)
    out1 = run(t["value"], t["loc_c"], t["loc_t"])
    v2 = torch.randn_like(t["value"])
    out2 = run(v2, t["loc_c"], t["loc_t"])
    out12 = run(t["value"] * 0.5 + v2 * 2.0, t["loc_c"], t["loc_t"])
    assert (out12 - (0.5 * out1 + 2.0 * out2)).abs().max().item() <= 1e-4
    # constant value = 1 and interior locations: out = sum of attention weights = 1 (joint softmax)
    lc = t["loc_c"].clamp(0.2, 0.8)
    lt = t["loc_t"].clamp(0.2, 0.8)
    ones = run(torch.ones_like(t["value"]), lc, lt)
    assert (ones - 1.0).abs().max().item() <= 1e-5
    # adjointness: <out(value), g> == <value, grad_value(g)>
    v = t["value"].clone().requires_grad_(True)
    out = run(v, t["loc_c"], t["loc_t"])
    (gv,) = torch.autograd.grad(out, v, t["grad_out"])
    lhs = (out.double() * t["grad_out"].double()).sum().item()
    rhs = (v.double() * gv.double()).sum().item()
    assert abs(lhs - rhs) <= 1e-4 * max(1.0, abs(lhs))


# ---------------------------------------------------------------------------------------------
# alternate backward routes (not the default dispatch) and larger BASELINE shapes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"MSDA_BWD_MODE": "atomic"},            # one-kernel backward, global float atomics
                                 {"MSDA_SCATTER_LDS_KB": "1"},           # no level row fits LDS -> "direct" branch
                                 {"MSDA_SCATTER_LDS_KB": "8"},           # many thin bands, straddling points
                                 {"MSDA_SCATTER_DBG": STATIC},           # static item order: the software pipeline
                                 {"MSDA_SCATTER_DBG": STATIC, "MSDA_SCATTER_LDS_KB": "8"},
                                 {"MSDA_BWD_CULL": "2"},                 # interval culling records (legacy scatter)
                                 {"MSDA_BWD_CULL": "2", "MSDA_SCATTER_DBG": STATIC},
                                 {"MSDA_BWD_CULL": "0"},                 # no culling table at all
                                 {"MSDA_SCATTER_OWN": "0"},             # LDS-atomic scatter instead of owner-computes
                                 {"MSDA_SCATTER_OWN": "0", "MSDA_SCATTER_DBG": STATIC},
                                 {"MSDA_FWD_RS": "1", "MSDA_BWD_RS": "1"},                       # resident-slab gather pass on a tiny shape
                                 {"MSDA_FWD_RS": "1", "MSDA_BWD_RS": "1", "MSDA_SCATTER_DBG": STATIC},
                                 # the other route bits of MSDA_SCATTER_DBG (csrc/msda_params.h: a route bit keeps the results).  The
                                 # temporal case below has two one-band levels and a static stride that shares a factor with them: its
                                 # bands rotate under the static order alone and stay put with kSdbgNoBandRotation added
                                 {"MSDA_SCATTER_DBG": str(kSdbgStaticStride | kSdbgNoBandRotation)},
                                 {"MSDA_SCATTER_DBG": str(kSdbgSeparateZero)},       # the zero-fill as a launch of its own
                                 {"MSDA_SCATTER_DBG": str(kSdbgNoFourSlotRule)}])    # five pixels per owner quad on a few-item call
def test_backward_alternate_routes(env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g, d = _golden_dict("op_devis_small")
    out, gv, gl, ga = _run_op(d, torch.float32)
    assert _maxabs(gv, g["grad_value"]) <= 2e-5 * max(1.0, np.abs(g["grad_value"]).max())
    assert _maxabs(gl, g["grad_sampling_loc"]) <= 2e-5 * max(1.0, np.abs(g["grad_sampling_loc"]).max())
    assert _maxabs(ga, g["grad_attn_weight"]) <= 2e-5 * max(1.0, np.abs(g["grad_attn_weight"]).max())
    dt = make_temporal_inputs(41, T=4, W=3, M=8, D=32, Lq=23, shapes=[(9, 7), (5, 4)], Pc=4, Pt=2)
    ref = temporal_reference(*(np.asarray(dt[k], dtype=np.float64) if dt[k].dtype.kind == "f" else dt[k]
                               for k in ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out")))
    got = _run_temporal(dt, torch.float32)
    for a, b in zip(got, ref):
        assert _maxabs(a, b) <= 2e-5 * max(1.0, np.abs(b).max())
    if env == {"MSDA_SCATTER_DBG": str(kSdbgSeparateZero)}:
        # the bit is what it is named after: the route names the zero-fill launch with it and not without it
        t = [torch.from_numpy(dt[k]).to(DEV) for k in ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out")]
        with_bit = _direct_temporal_backward_route(*t, 1)
        monkeypatch.delenv("MSDA_SCATTER_DBG")
        without = _direct_temporal_backward_route(*t, 1)
        assert "owner-computes" in with_bit and "zero-fill of pixels outside the bands" in with_bit, with_bit
        assert "owner-computes" in without and "zero-fill" not in without, without


def test_backward_without_workspace_static_schedule():
    """The C ABI allows workspace = NULL (static item stride)."""
    from devis_amd import _native
    g, d = _golden_dict("op_devis_small")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items()}
    gv = torch.full(t["value"].shape, float("nan"), device=DEV)        # ABI v4: overwritten, not accumulated
    gl, ga = torch.empty_like(t["loc"]), torch.empty_like(t["aw"])
    N, S, M, D = t["value"].shape
    _, Lq, _, L, P, _ = t["loc"].shape
    lib = _native.load()
    rc = lib.msda_backward(0, t["value"].data_ptr(), t["shapes"].data_ptr(), t["lsi"].data_ptr(), t["loc"].data_ptr(),
                           t["aw"].data_ptr(), t["grad_out"].float().contiguous().data_ptr(), N, S, M, D, L, Lq, P,
                           gv.data_ptr(), 0, gl.data_ptr(), ga.data_ptr(), None, 0, None, None,
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert _maxabs(gv.double().cpu().numpy(), g["grad_value"]) <= 2e-5 * max(1.0, np.abs(g["grad_value"]).max())


def test_many_levels_falls_back_to_atomic_kernel():
    """L > 32 levels: the LDS scatter declines, the one-kernel backward takes over."""
    shapes = [(3, 2), (2, 2)] * 20          # 40 levels
    d = make_inputs(55, 1, 4, 16, 9, shapes, 2, "wide", np.float32)
    ref = oracle_fwd_bwd(d, np.float32)
    got = _run_op(d, torch.float32)
    assert _maxabs(got[0], ref[0]) <= 1e-6
    for a, b in zip(got[1:], ref[1:]):
        assert _maxabs(a, b) <= 2e-5 * max(1.0, np.abs(b).max())


def test_full_size_cfg2_encoder_bf16_properties():
    """BASELINE configs[1]: single-frame Deformable-DETR encoder attention on the 800x1333 pyramid,
    Lq = S = 22223, M=8, K=4, C=256, bf16 -- checked through size-independent properties plus an
    oracle comparison on a random subset of query rows."""
    from devis_amd.functions import MSDeformAttnFunction
    from helpers import PYR_B
    from oracle import msda_oracle as O
    shapes_np = np.asarray(PYR_B, dtype=np.int64)
    S = int((shapes_np[:, 0] * shapes_np[:, 1]).sum())
    g = torch.Generator().manual_seed(9)
    value = (torch.rand(1, S, 8, 32, generator=g) * 2 - 1).to(torch.bfloat16)
    loc = (torch.rand(1, S, 8, 4, 4, 2, generator=g) * 1.2 - 0.1).to(torch.bfloat16)
    aw = torch.softmax(torch.randn(1, S, 8, 16, generator=g), -1).view(1, S, 8, 4, 4).to(torch.bfloat16)
    go = torch.randn(1, S, 256, generator=g).to(torch.bfloat16)
    shapes = torch.from_numpy(shapes_np).to(DEV)
    lsi = torch.from_numpy(O.level_start_index(shapes_np)).to(DEV)
    v, l, a = (x.to(DEV).requires_grad_(True) for x in (value, loc, aw))
    out = MSDeformAttnFunction.apply(v, shapes, lsi, l, a, 64)
    gv, gl, ga = torch.autograd.grad(out, (v, l, a), go.to(DEV))
    torch.cuda.synchronize()
    # oracle on 64 random query rows (forward + grad_loc/grad_attn are row-local)
    rows = torch.randperm(S, generator=g)[:64]
    sub = lambda x: x[:, rows].double().numpy()
    o_ref = O.forward(value.double().numpy(), shapes_np, O.level_start_index(shapes_np), sub(loc), sub(aw))
    assert _maxabs(out[:, rows].detach().double().cpu().numpy(), o_ref) <= 1e-2
    _, gl_ref, ga_ref = O.backward(value.double().numpy(), shapes_np, O.level_start_index(shapes_np), sub(loc), sub(aw),
                                   go[:, rows].double().numpy())
    assert _maxabs(ga[:, rows].double().cpu().numpy(), ga_ref) <= 2e-2 * max(1.0, np.abs(ga_ref).max())
    assert _maxabs(gl[:, rows].double().cpu().numpy(), gl_ref) <= 2e-2 * max(1.0, np.abs(gl_ref).max())
    # adjointness ties grad_value to the forward:  <out(value), g> == <value, grad_value(g)>
    lhs = (out.detach().double() * go.to(DEV).double()).sum().item()
    rhs = (v.detach().double() * gv.double()).sum().item()
    assert abs(lhs - rhs) <= 2e-2 * max(1.0, abs(lhs))


def test_full_size_temporal_encoder_800x1333():
    """Largest realistic call: fused temporal ENCODER attention on the 800x1333 pyramid, T=6, Lq = S = 22223
    per frame (133 338 rows, 96 taps each), local sampling.  Forward / grad_loc / grad_attn are row-local and
    are compared with the oracle (reference call pattern) on sampled rows; grad_value through adjointness
    AND directly: the oracle's grad_value of ONE head (all frames, all 133 k rows; the heads are independent), on the
    scatter's image-order item schedule."""
    from devis_amd.functions import MSDeformAttnTemporalFunction
    from helpers import PYR_B
    from oracle import msda_oracle as O
    T, W, M, D, L, P = 6, 5, 8, 32, 4, 4
    shapes_np = np.asarray(PYR_B, dtype=np.int64)
    S = int((shapes_np[:, 0] * shapes_np[:, 1]).sum())
    g = torch.Generator().manual_seed(5)
    centres = torch.cat([torch.stack(torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w,
                                                     indexing="ij"), -1).reshape(-1, 2).flip(-1) for h, w in PYR_B], 0)
    wh = torch.from_numpy(shapes_np[:, ::-1].copy()).float()
    ref = centres[None, :, None, None, None, :]
    value = torch.rand(T, S, M, D, generator=g) * 2 - 1
    loc_c = ref + torch.randn(T, S, M, L, P, 2, generator=g) * 2.0 / wh[None, None, None, :, None, :]
    loc_t = ref + torch.randn(T, S, M, W * L, P, 2, generator=g) * 2.0 / wh.repeat(W, 1)[None, None, None, :, None, :]
    aw = torch.softmax(torch.randn(T, S, M, L * P * (1 + W), generator=g), -1)
    aw_c = aw[..., :L * P].reshape(T, S, M, L, P).contiguous()
    aw_t = aw[..., L * P:].reshape(T, S, M, W * L, P).contiguous()
    go = torch.randn(T, S, M * D, generator=g)
    ftab_np = np.array([[f for f in range(T) if f != t] for t in range(T)], dtype=np.int32)
    dev = lambda x: x.to(DEV).contiguous().requires_grad_(x.is_floating_point())
    v, lc, ac, lt, at = dev(value), dev(loc_c), dev(aw_c), dev(loc_t), dev(aw_t)
    shapes = torch.from_numpy(shapes_np).to(DEV)
    lsi_np = O.level_start_index(shapes_np)
    out = MSDeformAttnTemporalFunction.apply(v, shapes, torch.from_numpy(lsi_np).to(DEV), torch.from_numpy(ftab_np).to(DEV),
                                             lc, ac, lt, at, 1)
    gv, glc, gac, glt, gat = torch.autograd.grad(out, (v, lc, ac, lt, at), go.to(DEV))
    torch.cuda.synchronize()
    rows = torch.randperm(S, generator=g)[:24]
    sub = lambda x: np.ascontiguousarray(x[:, rows].double().numpy())
    vd = value.double().numpy()
    r = temporal_reference(vd, shapes_np, lsi_np, ftab_np, sub(loc_c), sub(aw_c), sub(loc_t), sub(aw_t), sub(go))
    # grad_loc is discontinuous at pixel borders: compare it with the oracle in the SAME (fp32) arithmetic
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    r32 = temporal_reference(f32(vd), shapes_np, lsi_np, ftab_np, f32(sub(loc_c)), f32(sub(aw_c)), f32(sub(loc_t)),
                             f32(sub(aw_t)), f32(sub(go)))
    pick = lambda x: x.detach()[:, rows].double().cpu().numpy()
    assert _maxabs(pick(out), r[0]) <= 1e-5
    for got, want in ((pick(glc), r32[2]), (pick(gac), r[3]), (pick(glt), r32[4]), (pick(gat), r[5])):
        assert _maxabs(got, want) <= 1e-3 * max(1.0, np.abs(want).max())
    lhs = (out.detach().double() * go.to(DEV).double()).sum().item()
    rhs = (v.detach().double() * gv.double()).sum().item()
    assert abs(lhs - rhs) <= 1e-5 * max(1.0, abs(lhs))
    # grad_value of head 5 against the oracle run on that head alone (value / points / grad_out channels of the head)
    assert "items in image order" in _direct_temporal_backward_route(v, shapes, torch.from_numpy(lsi_np).to(DEV), torch.from_numpy(ftab_np).to(DEV),
                                                                     lc, ac, lt, at, go.to(DEV), 1)
    h = 5
    one = lambda x: np.ascontiguousarray(x[:, :, h:h + 1].double().numpy())
    rh = temporal_reference(one(value), shapes_np, lsi_np, ftab_np, one(loc_c), one(aw_c), one(loc_t), one(aw_t),
                            np.ascontiguousarray(go[:, :, h * D:(h + 1) * D].double().numpy()))
    err = _maxabs(gv[:, :, h].double().cpu().numpy(), rh[1][:, :, 0])
    assert err <= 2e-5 * max(1.0, np.abs(rh[1]).max()), err


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 1e-2), (torch.float16, 2e-3), (torch.float32, 2e-5)], ids=["bf16", "f16", "f32"])
def test_image_order_scatter_on_a_batch_of_clips(dtype, tol):
    """The scatter's image-order item schedule (long temporal calls: Lq >= 8192, frames > 1) on a BATCH of 4 clips in the
    16-bit storage types (grad_value written in the storage type) and in fp32: grad_value, outputs and the other gradients
    directly against the oracle, clip by clip."""
    from devis_amd.functions import MSDeformAttnTemporalFunction
    shapes = [(66, 96), (33, 48), (17, 24), (9, 12)]          # S = 8436 >= 8192
    S = int(sum(hh * ww for hh, ww in shapes))
    clips, T, M = 4, 2, 2
    keys = ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out")
    ds, refs = [], []
    for c in range(clips):
        d = make_temporal_inputs(100 + c, T=T, W=T - 1, M=M, D=32, Lq=S, shapes=shapes, Pc=4, Pt=4)
        if c % 2 == 0:      # encoder-like locality for half of the clips, range-wide sampling for the others
            d["loc_c"] = localise(d["loc_c"], shapes, 2.0, 1 + c)
            d["loc_t"] = localise(d["loc_t"], shapes, 2.0, 50 + c)
        d = round_to({k: (np.asarray(v, dtype=np.float64) if v.dtype.kind == "f" else v) for k, v in d.items()}, dtype)
        ds.append(d)
        refs.append(temporal_reference(*(d[k] for k in keys)))
    cat = lambda k: torch.from_numpy(np.concatenate([d[k] for d in ds], 0)).to(DEV, dtype).requires_grad_(True)
    leaves = [cat(k) for k in ("value", "loc_c", "aw_c", "loc_t", "aw_t")]
    d0 = ds[0]
    out = MSDeformAttnTemporalFunction.apply(leaves[0], torch.from_numpy(d0["shapes"]).to(DEV), torch.from_numpy(d0["lsi"]).to(DEV),
                                             torch.from_numpy(d0["ftab"]).to(DEV), *leaves[1:], clips)
    grads = torch.autograd.grad(out, leaves, cat("grad_out").detach())
    route = _direct_temporal_backward_route(leaves[0], torch.from_numpy(d0["shapes"]).to(DEV), torch.from_numpy(d0["lsi"]).to(DEV),
                                            torch.from_numpy(d0["ftab"]).to(DEV), *leaves[1:], cat("grad_out").detach(), clips)
    assert "items in image order" in route and ("storage type" in route) == (dtype != torch.float32), route
    scale = lambda x: max(1.0, float(np.abs(x).max()))
    for c in range(clips):
        sl = slice(c * T, (c + 1) * T)
        assert _maxabs(out.detach()[sl].double().cpu().numpy(), refs[c][0]) <= tol * scale(refs[c][0]), c
        # grad_value DIRECTLY (not through adjointness), then grad_attn of both point sets
        err = _maxabs(grads[0][sl].double().cpu().numpy(), refs[c][1])
        assert err <= 2 * tol * scale(refs[c][1]), (c, err)
        for i in (2, 4):
            err = _maxabs(grads[i][sl].double().cpu().numpy(), refs[c][1 + i])
            assert err <= 3 * tol * scale(refs[c][1 + i]), (c, i, err)


def test_forward_resident_slab_kernel_forced(monkeypatch):
    """MSDA_FWD_RS=1 forces the resident-slab forward (levels 1.. of a source frame in a workgroup-shared LDS slab) on
    shapes the host heuristic would leave to the tile kernel (fixtures with D != 32 stay there)."""
    monkeypatch.setenv("MSDA_FWD_RS", "1")
    for name in ("op_devis_small", "op_batched_im2col", "op_out_of_range", "op_many_levels", "op_cfg1", "op_generic_D64"):
        g, d = _golden_dict(name)
        out, gv, gl, ga = _run_op(d, torch.float32)
        assert _maxabs(out, g["out"]) <= 1e-6, name
    ftab = np.array([[1, 1], [0, 2], [1, 3], [2, 4], [3, 3]], dtype=np.int32)     # repeated frames
    for kw in (dict(T=4, W=3, ftab=None, Lq=37), dict(T=5, W=2, ftab=ftab, Lq=150)):
        dt = make_temporal_inputs(47, kw["T"], kw["W"], 8, 32, kw["Lq"], [(9, 7), (5, 4), (3, 2)], 4, 2, ftab=kw["ftab"])
        ref = temporal_reference(*(np.asarray(dt[k], dtype=np.float64) if dt[k].dtype.kind == "f" else dt[k]
                                   for k in ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t")))
        got = _run_temporal(dt, torch.float32)
        assert _maxabs(got[0], ref) <= 2e-5 * max(1.0, np.abs(ref).max())



def test_backward_resident_slab_kernel_forced(monkeypatch):
    """MSDA_BWD_RS=1 forces the resident-slab gather pass on small shapes."""
    monkeypatch.setenv("MSDA_BWD_RS", "1")
    for name in ("op_devis_small", "op_batched_im2col", "op_out_of_range", "op_many_levels", "op_cfg1"):
        g, d = _golden_dict(name)
        out, gv, gl, ga = _run_op(d, torch.float32)
        assert _maxabs(gv, g["grad_value"]) <= 2e-5 * max(1.0, np.abs(g["grad_value"]).max()), name
        assert _maxabs(gl, g["grad_sampling_loc"]) <= 2e-5 * max(1.0, np.abs(g["grad_sampling_loc"]).max()), name
        assert _maxabs(ga, g["grad_attn_weight"]) <= 2e-5 * max(1.0, np.abs(g["grad_attn_weight"]).max()), name
    ftab = np.array([[1, 1], [0, 2], [1, 3], [2, 4], [3, 3]], dtype=np.int32)
    for kw in (dict(T=4, W=3, ftab=None, Lq=37), dict(T=5, W=2, ftab=ftab, Lq=150)):
        dt = make_temporal_inputs(49, kw["T"], kw["W"], 8, 32, kw["Lq"], [(9, 7), (5, 4), (3, 2)], 4, 2, ftab=kw["ftab"])
        ref = temporal_reference(*(np.asarray(dt[k], dtype=np.float64) if dt[k].dtype.kind == "f" else dt[k]
                                   for k in ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out")))
        got = _run_temporal(dt, torch.float32)
        for a, b in zip(got, ref):
            assert _maxabs(a, b) <= 2e-5 * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("route", ["points", "intervals", "lds_atomics", "atomic", "generic", "direct_levels", "no_workspace"])
def test_grad_value_is_overwritten(route, monkeypatch):
    """ABI v4: grad_value need not be zeroed -- every backward route overwrites (or zero-fills) all of it,
    including pixel rows of `value` that belong to no level (spatial_shapes not tiling [0, S))."""
    from devis_amd import _native
    if route == "intervals":
        monkeypatch.setenv("MSDA_BWD_CULL", "2")
    if route == "lds_atomics":
        monkeypatch.setenv("MSDA_SCATTER_OWN", "0")
    if route == "atomic":
        monkeypatch.setenv("MSDA_BWD_MODE", "atomic")
    if route == "generic":
        monkeypatch.setenv("MSDA_FORCE_GENERIC", "1")
    if route == "direct_levels":
        monkeypatch.setenv("MSDA_SCATTER_LDS_KB", "2")          # LDS-atomic scatter, no level row fits: float-atomic branch
    rng = np.random.default_rng(5)
    shapes = [(9, 7), (5, 4), (3, 2)]
    d = make_inputs(5, 3, 8, 32, 41, shapes, 4)
    pad = 5                                                       # rows of value outside every level
    value = np.concatenate([d["value"], rng.standard_normal((3, pad, 8, 32))], axis=1)
    ref = oracle_fwd_bwd(d)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items()}
    v = torch.from_numpy(value).float().to(DEV)
    loc, aw, go = t["loc"].float(), t["aw"].float(), t["grad_out"].float().contiguous()
    gv = torch.full(v.shape, float("nan"), device=DEV)
    gl, ga = torch.empty_like(loc), torch.empty_like(aw)
    if route == "no_workspace":
        N, S, M, D = v.shape
        _, Lq, _, L, P, _ = loc.shape
        rc = _native.load().msda_backward(0, v.data_ptr(), t["shapes"].data_ptr(), t["lsi"].data_ptr(), loc.data_ptr(),
                                          aw.data_ptr(), go.data_ptr(), N, S, M, D, L, Lq, P, gv.data_ptr(), 0,
                                          gl.data_ptr(), ga.data_ptr(), None, 0, None, None,
                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    else:
        _native.backward(v, t["shapes"], t["lsi"], loc, aw, go, gv, gl, ga)
    got = gv.cpu().numpy()
    S0 = d["value"].shape[1]
    assert np.isfinite(got).all()
    assert (got[:, S0:] == 0).all()
    assert _maxabs(got[:, :S0], ref[1]) <= 2e-5 * max(1.0, np.abs(ref[1]).max())


def test_a_stale_shapes_hint_poisons_grad_value_instead_of_returning_wrong_sums():
    """include/msda.h: for a backward call the host copy of the shapes must be a true copy.  A raw C-ABI caller whose hint
    hides a level wider than a scatter band (1024 pixels per row) gets that level's grad_value as NaN -- loud -- and not
    sums added into a buffer nobody zeroed; with the true hint (or none) the same call is exact."""
    import ctypes
    from devis_amd import _native
    shapes = [(2, 1100), (3, 5)]
    d = make_inputs(9, 1, 2, 32, 23, shapes, 4)
    ref = oracle_fwd_bwd(d)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items()}
    v = t["value"].float().contiguous()
    loc, aw, go = t["loc"].float(), t["aw"].float(), t["grad_out"].float().contiguous()
    N, S, M, D = v.shape
    _, Lq, _, L, P, _ = loc.shape
    ws = _native.bwd_workspace(v.device, N, Lq, M, L)

    def call(hint):
        gv = torch.full(v.shape, 123.0, device=DEV)
        gl, ga = torch.empty_like(loc), torch.empty_like(aw)
        rc = _native.load().msda_backward(0, v.data_ptr(), t["shapes"].data_ptr(), t["lsi"].data_ptr(), loc.data_ptr(),
                                          aw.data_ptr(), go.data_ptr(), N, S, M, D, L, Lq, P, gv.data_ptr(), 0,
                                          gl.data_ptr(), ga.data_ptr(), ws.data_ptr(), ws.numel() * 4, None, hint,
                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        return gv.cpu().numpy()

    true_hint = (ctypes.c_int64 * 4)(2, 1100, 3, 5)
    for hint in (true_hint, None):
        got = call(hint)
        assert _maxabs(got, ref[1]) <= 1e-4 * max(1.0, np.abs(ref[1]).max())        # (float atomics on the wide level)
    stale = (ctypes.c_int64 * 4)(2, 100, 3, 5)
    got = call(stale)
    assert np.isnan(got[:, :2200]).all()                                         # the hidden wide level: poisoned
    assert _maxabs(got[:, 2200:], ref[1][:, 2200:]) <= 1e-4 * max(1.0, np.abs(ref[1]).max())      # the others: as before


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_storage_typed_grad_value_is_overwritten_outside_the_levels(dtype):
    """The same contract for a 16-bit grad_value written by the scatter itself (ABI v10): pixel rows of `value` that belong to
    no level come back as zeros (round 4: from the scatter kernel's own prologue when the host knows the shapes)."""
    from devis_amd import _native
    rng = np.random.default_rng(6)
    shapes = [(9, 7), (5, 4), (3, 2)]
    d = round_to(make_inputs(6, 3, 8, 32, 41, shapes, 4), dtype)
    pad = 7
    value = np.concatenate([d["value"], rng.standard_normal((3, pad, 8, 32))], axis=1)
    ref = oracle_fwd_bwd(d)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items()}
    v = torch.from_numpy(value).to(DEV, dtype)
    loc, aw, go = t["loc"].to(dtype), t["aw"].to(dtype), t["grad_out"].to(dtype).contiguous()
    gvt = _native.grad_value_dtype(v, t["shapes"], 41, 3, 4)
    assert gvt == dtype
    gv = torch.full(v.shape, float("nan"), device=DEV, dtype=gvt)
    gl, ga = torch.empty_like(loc), torch.empty_like(aw)
    _native.backward(v, t["shapes"], t["lsi"], loc, aw, go, gv, gl, ga)
    assert "owner-computes" in _native.last_route() and "zero-fill" not in _native.last_route(), _native.last_route()
    got = gv.float().cpu().numpy()
    S0 = d["value"].shape[1]
    assert np.isfinite(got).all()
    assert (got[:, S0:] == 0).all()
    assert _maxabs(got[:, :S0], ref[1]) <= 2e-2 * max(1.0, np.abs(ref[1]).max())


@pytest.mark.parametrize("route", ["default", "tile", "atomic", "generic"])
def test_head_major_value_layout(route, monkeypatch):
    """value stored head-major ([M, N, S, D] memory behind the same [N, S, M, D] shape; include/msda.h
    value_strides): same results, grad_value comes back dense."""
    from devis_amd import _native
    from devis_amd.functions import MSDeformAttnFunction
    if route == "tile":
        monkeypatch.setenv("MSDA_FWD_RS", "0"); monkeypatch.setenv("MSDA_BWD_RS", "0")
    if route == "default":
        monkeypatch.setenv("MSDA_FWD_RS", "1"); monkeypatch.setenv("MSDA_BWD_RS", "1")
    if route == "atomic":
        monkeypatch.setenv("MSDA_BWD_MODE", "atomic")
    if route == "generic":
        monkeypatch.setenv("MSDA_FORCE_GENERIC", "1")
    g, d = _golden_dict("op_batched_im2col")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items()}
    # dense rows padded by one head slot (what devis_amd.functions.project_value produces)
    vd = t["value"].float()
    buf = torch.full((vd.shape[0], vd.shape[1], vd.shape[2] + 1, vd.shape[3]), float("nan"), device=DEV)
    buf[:, :, :vd.shape[2]] = vd
    vp = buf[:, :, :vd.shape[2]].requires_grad_(True)
    loc0, aw0 = t["loc"].float().requires_grad_(True), t["aw"].float().requires_grad_(True)
    outp = MSDeformAttnFunction.apply(vp, t["shapes"], t["lsi"], loc0, aw0, 3)
    gp = torch.autograd.grad(outp, (vp, loc0, aw0), t["grad_out"].float())
    for got, key in zip((outp,) + gp, ("out", "grad_value", "grad_sampling_loc", "grad_attn_weight")):
        assert _maxabs(got.detach().cpu().numpy(), g[key]) <= 2e-5 * max(1.0, np.abs(g[key]).max()), key
    v = _native.head_major(t["value"].float()).requires_grad_(True)
    assert not v.is_contiguous()
    loc, aw = t["loc"].float().requires_grad_(True), t["aw"].float().requires_grad_(True)
    out = MSDeformAttnFunction.apply(v, t["shapes"], t["lsi"], loc, aw, 2)
    gv, gl, ga = torch.autograd.grad(out, (v, loc, aw), t["grad_out"].float())
    assert gv.shape == v.shape
    for got, key in ((out, "out"), (gv, "grad_value"), (gl, "grad_sampling_loc"), (ga, "grad_attn_weight")):
        assert _maxabs(got.detach().cpu().numpy(), g[key]) <= 2e-5 * max(1.0, np.abs(g[key]).max()), key
    # fused temporal op on a head-major clip batch
    dt = make_temporal_inputs(49, 4, 3, 8, 32, 37, [(9, 7), (5, 4), (3, 2)], 4, 2)
    ref = temporal_reference(*(np.asarray(dt[k], dtype=np.float64) if dt[k].dtype.kind == "f" else dt[k]
                               for k in ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out")))
    got = _run_temporal(dt, torch.float32, head_major=True)
    for a, b in zip(got, ref):
        assert _maxabs(a, b) <= 2e-5 * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("env", [{}, {"MSDA_SCATTER_DBG": STATIC}, {"MSDA_BWD_CULL": "2"}])
def test_scatter_survivor_list_overflow(env, monkeypatch):
    """More surviving points per cull batch than the survivor list holds (dense single-band levels, long
    candidate ranges): the prefix-scan-and-retry path, in dynamic and static item order."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = make_inputs(77, 2, 8, 32, 2600, [(6, 5), (3, 3)], 4, "unit", np.float32)
    ref = oracle_fwd_bwd(d, np.float64)
    ref32 = oracle_fwd_bwd(d, np.float32)      # grad_loc: same-arithmetic oracle (cell borders, see above)
    out, gv, gl, ga = _run_op(d, torch.float32)
    assert _maxabs(out, ref[0]) <= 1e-5
    assert _maxabs(gv, ref32[1]) <= 1e-4 * max(1.0, np.abs(ref[1]).max())
    assert _maxabs(gl, ref32[2]) <= 1e-4 * max(1.0, np.abs(ref32[2]).max())
    assert _maxabs(ga, ref32[3]) <= 1e-4 * max(1.0, np.abs(ref[3]).max())


def test_bench_scale_batch_equals_single_clip_runs():
    """The bench workload (16 cfg3 clips in one fused call: slab kernels, static-order pipelined scatter)
    against the same clips run one at a time (tile kernels, dynamic tickets): every output and gradient of
    every clip must agree -- a size-independent cross-check of the two dispatch regimes at full size."""
    from devis_amd.functions import MSDeformAttnTemporalFunction
    clips, T, Lq = 16, 6, 300
    ds = [make_temporal_inputs(900 + c, T=T, W=5, M=8, D=32, Lq=Lq, shapes=PYR_A, Pc=4, Pt=4) for c in range(clips)]
    shapes = torch.from_numpy(ds[0]["shapes"]).to(DEV)
    lsi = torch.from_numpy(ds[0]["lsi"]).to(DEV)
    ftab = torch.from_numpy(ds[0]["ftab"]).to(DEV)
    keys = ("value", "loc_c", "aw_c", "loc_t", "aw_t")

    def run(sel):
        leaves = [torch.from_numpy(np.concatenate([ds[c][k] for c in sel], 0)).to(DEV).requires_grad_(True) for k in keys]
        go = torch.from_numpy(np.concatenate([ds[c]["grad_out"] for c in sel], 0)).to(DEV)
        out = MSDeformAttnTemporalFunction.apply(leaves[0], shapes, lsi, ftab, *leaves[1:], len(sel))
        grads = torch.autograd.grad(out, leaves, go)
        return [out.detach()] + [g.detach() for g in grads]

    batch = run(list(range(clips)))
    for c in (0, 7, 15):
        single = run([c])
        for b, s in zip(batch, single):
            bc = b[c * T:(c + 1) * T]
            scale = max(1.0, s.abs().max().item())
            assert (bc - s).abs().max().item() <= 2e-6 * scale


@pytest.mark.parametrize("local", [False, True])
def test_long_candidate_range_block_summaries(local):
    """Lq large enough (> 4 cull batches of 2048 groups) for the 64-query block summaries and the batch-skipping
    pre-pass of the scatter: uniform locations (every batch live) and query-index-local ones (most skipped)."""
    d = make_inputs(314, 1, 8, 32, 11000, [(40, 24), (20, 12), (10, 6)], 4, "unit", np.float32)
    if local:
        rng = np.random.default_rng(9)
        q = np.arange(11000, dtype=np.float64) / 11000.0
        y = q[None, :, None, None, None] + rng.normal(0, 0.02, size=d["loc"].shape[:-1])
        d["loc"][..., 1] = np.clip(y, -0.1, 1.1).astype(np.float32)
    ref = oracle_fwd_bwd(d, np.float64)
    ref32 = oracle_fwd_bwd(d, np.float32)
    out, gv, gl, ga = _run_op(d, torch.float32)
    assert _maxabs(out, ref[0]) <= 1e-5
    assert _maxabs(gv, ref32[1]) <= 1e-4 * max(1.0, np.abs(ref[1]).max())
    assert _maxabs(gl, ref32[2]) <= 1e-4 * max(1.0, np.abs(ref32[2]).max())
    assert _maxabs(ga, ref32[3]) <= 1e-4 * max(1.0, np.abs(ref[3]).max())


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 1e-2), (torch.float16, 2e-3)], ids=["bf16", "f16"])
def test_grad_value_in_the_storage_type(dtype, tol, monkeypatch):
    """ABI v10: for 16-bit storage the owner-computes scatter writes grad_value directly in the storage type
    (msda_grad_value_dtype says where); the result equals the fp32 buffer of the same call rounded once.  Where another
    route produces grad_value (D = 64 here, or the LDS-atomic scatter) the query answers fp32, and a storage-typed buffer
    is refused instead of being filled wrongly."""
    from devis_amd import _native
    d = round_to(make_inputs(31, 2, 8, 32, 77, [(12, 20), (6, 10), (3, 5)], 4, "wide", np.float64, value_scale=1.0), dtype)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items()}
    v, loc, aw, go = (t[k].to(dtype) for k in ("value", "loc", "aw", "grad_out"))
    assert _native.grad_value_dtype(v, t["shapes"], 77, 3, 4) == dtype
    ref = oracle_fwd_bwd(d, np.float64)
    outs = {}
    for gdt in (torch.float32, dtype):
        gv = torch.full(v.shape, float("nan"), dtype=gdt, device=DEV)
        gl, ga = torch.empty_like(loc), torch.empty_like(aw)
        _native.backward(v, t["shapes"], t["lsi"], loc, aw, go, gv, gl, ga)
        torch.cuda.synchronize()
        assert ("storage type" in _native.last_route()) == (gdt == dtype), _native.last_route()
        outs[gdt] = gv
        assert _maxabs(gv.double().cpu().numpy(), ref[1]) <= tol * max(1.0, np.abs(ref[1]).max())
    # the same sums (up to the order of a pixel's terms, which is list order: the last bits of an fp32 sum vary from run to
    # run), rounded once on the way out: within one unit of the storage type's last place
    ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    a, b = outs[torch.float32].double(), outs[dtype].double()
    assert float(((a - b).abs() - ulp * a.abs()).max()) <= 1e-6
    # other routes: fp32 only
    v64 = torch.zeros((2, v.shape[1], 4, 64), dtype=dtype, device=DEV)
    assert _native.grad_value_dtype(v64, t["shapes"], 77, 3, 4) == torch.float32
    monkeypatch.setenv("MSDA_SCATTER_OWN", "0")
    assert _native.grad_value_dtype(v, t["shapes"], 77, 3, 4) == torch.float32
    gv = torch.empty(v.shape, dtype=dtype, device=DEV)
    with pytest.raises(RuntimeError, match="grad_value"):
        _native.backward(v, t["shapes"], t["lsi"], loc, aw, go, gv, torch.empty_like(loc), torch.empty_like(aw))


def test_graph_replay_equals_eager():
    """The library only enqueues work -- no allocation of its own, no synchronisation (include/msda.h) -- so forward +
    backward of the call DeVIS issues per decoder layer (one clip; main.py:85, tracker.py:320-323) can be captured in a
    HIP graph; replays on new input values reproduce the eager results (grad_value up to the order of a pixel's terms)."""
    from devis_amd.functions import MSDeformAttnTemporalFunction
    d = make_temporal_inputs(77, T=6, W=5, M=8, D=32, Lq=300, shapes=PYR_A, Pc=4, Pt=4)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}
    keys = ("value", "loc_c", "aw_c", "loc_t", "aw_t")
    static = [t[k].clone().requires_grad_(True) for k in keys]

    def step():
        out = MSDeformAttnTemporalFunction.apply(static[0], t["shapes"], t["lsi"], t["ftab"], *static[1:], 1)
        return (out,) + torch.autograd.grad(out, static, t["grad_out"])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()                                  # warm-up: LDS opt-ins, host copy of the shapes, allocator
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for seed in (78, 79):                           # new values in the captured input buffers
        d2 = make_temporal_inputs(seed, T=6, W=5, M=8, D=32, Lq=300, shapes=PYR_A, Pc=4, Pt=4)
        with torch.no_grad():
            for buf, k in zip(static, keys):
                buf.copy_(torch.from_numpy(d2[k]).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in captured]
        want = step()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(got, want)):
            if i == 1:      # grad_value: fp32 sums in list order
                assert _maxabs(a.double().cpu().numpy(), b.double().cpu().numpy()) <= 1e-5 * max(1.0, float(b.abs().max()))
            else:
                assert torch.equal(a, b), i


def test_capture_with_a_spatial_shapes_tensor_never_seen_before():
    """The reference's transformer rebuilds ``spatial_shapes`` on every forward (deformable_transformer.py:87).  A tensor the
    library has no host copy of cannot be read back inside a HIP-graph capture: the call then goes without the hint
    (`_native.shapes_hint` returns None) instead of breaking the capture, and the replay equals the eager call."""
    from devis_amd import _native
    from devis_amd.functions import MSDeformAttnTemporalFunction
    d = make_temporal_inputs(81, T=3, W=2, M=8, D=32, Lq=50, shapes=[(20, 33), (10, 17), (5, 9), (3, 5)], Pc=4, Pt=4)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}
    keys = ("value", "loc_c", "aw_c", "loc_t", "aw_t")
    static = [t[k].clone().requires_grad_(True) for k in keys]

    def step(shapes):
        out = MSDeformAttnTemporalFunction.apply(static[0], shapes, t["lsi"], t["ftab"], *static[1:], 1)
        return (out,) + torch.autograd.grad(out, static, t["grad_out"])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(t["shapes"])
    torch.cuda.current_stream().wait_stream(side)
    fresh = t["shapes"].clone()                     # same values, a tensor the hint cache has not seen
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert _native.shapes_hint(fresh) is None
        captured = step(fresh)
    graph.replay()
    torch.cuda.synchronize()
    want = step(t["shapes"])
    for i, (a, b) in enumerate(zip(captured, want)):
        assert _maxabs(a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()) <= 1e-5 * max(1.0, float(b.abs().max())), i


@pytest.mark.parametrize("env", [{}, {"MSDA_FWD_RS": "1", "MSDA_BWD_RS": "1"}, {"MSDA_FORCE_GENERIC": "1"}, {"MSDA_SCATTER_OWN": "0"},
                                 {"MSDA_BWD_MODE": "atomic"}],
                         ids=["auto", "resident-slab", "generic", "lds-scatter", "atomic"])
@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 1e-2), (torch.float16, 2e-3)], ids=["bf16", "f16"])
def test_fp32_sampling_beside_a_16_bit_value(dtype, tol, env, monkeypatch):
    """ABI v11 (MSDA_BF16_LOC32 / MSDA_F16_LOC32): value / out / grad_out in 16 bits, sampling locations and attention
    weights -- and their gradients -- in float32, on every route, plain and fused temporal op, against the fp64 oracle on
    the same inputs (only value and grad_out rounded).  grad_loc / grad_attn come back in float32."""
    from devis_amd.functions import MSDeformAttnFunction, MSDeformAttnTemporalFunction
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    shapes = [(12, 20), (6, 10), (3, 5), (2, 3)]
    d = make_inputs(61, 2, 8, 32, 45, shapes, 4, "wide", np.float32, value_scale=1.0)
    d.update(round_to({k: np.asarray(d[k], dtype=np.float64) for k in ("value", "grad_out")}, dtype))
    ref = oracle_fwd_bwd(d, np.float64)
    ref32 = oracle_fwd_bwd({k: (np.asarray(v, dtype=np.float32) if v.dtype.kind == "f" else v) for k, v in d.items()}, np.float32)
    v = torch.from_numpy(np.asarray(d["value"], dtype=np.float64)).to(DEV, dtype).requires_grad_(True)
    loc = torch.from_numpy(d["loc"]).to(DEV).requires_grad_(True)
    aw = torch.from_numpy(d["aw"]).to(DEV).requires_grad_(True)
    assert loc.dtype == torch.float32
    out = MSDeformAttnFunction.apply(v, torch.from_numpy(d["shapes"]).to(DEV), torch.from_numpy(d["lsi"]).to(DEV), loc, aw, 64)
    go = torch.from_numpy(np.asarray(d["grad_out"], dtype=np.float64)).to(DEV, dtype)
    gv, gl, ga = torch.autograd.grad(out, (v, loc, aw), go)
    assert out.dtype == dtype and gv.dtype == dtype and gl.dtype == torch.float32 and ga.dtype == torch.float32
    scale = lambda x: max(1.0, float(np.abs(x).max()))
    npy = lambda t: t.detach().double().cpu().numpy()
    assert _maxabs(npy(out), ref[0]) <= tol * scale(ref[0])
    assert _maxabs(npy(gv), ref[1]) <= 2 * tol * scale(ref[1])
    assert _maxabs(npy(gl), ref32[2]) <= 1e-4 * scale(ref32[2])       # fp32 arithmetic on the same rounded value
    assert _maxabs(npy(ga), ref[3]) <= 1e-4 * scale(ref[3])
    # fused temporal op
    dt = make_temporal_inputs(62, T=3, W=2, M=8, D=32, Lq=40, shapes=shapes[:3], Pc=4, Pt=3)
    dt.update(round_to({k: np.asarray(dt[k], dtype=np.float64) for k in ("value", "grad_out")}, dtype))
    keys = ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out")
    tref = temporal_reference(*(np.asarray(dt[k], dtype=np.float64) if dt[k].dtype.kind == "f" else dt[k] for k in keys))
    f = lambda k, t: torch.from_numpy(np.asarray(dt[k], dtype=np.float64)).to(DEV, t).requires_grad_(True)
    tv = f("value", dtype)
    tl = [f(k, torch.float32) for k in ("loc_c", "aw_c", "loc_t", "aw_t")]
    tout = MSDeformAttnTemporalFunction.apply(tv, torch.from_numpy(dt["shapes"]).to(DEV), torch.from_numpy(dt["lsi"]).to(DEV),
                                              torch.from_numpy(dt["ftab"]).to(DEV), *tl, 1)
    tg = torch.autograd.grad(tout, [tv] + tl, torch.from_numpy(np.asarray(dt["grad_out"], dtype=np.float64)).to(DEV, dtype))
    got = [tout] + list(tg)
    for i, (a, b) in enumerate(zip(got, tref)):
        if i in (2, 4):
            continue        # grad_loc against an fp64 reference flips cells at pixel borders (checked above against fp32)
        assert _maxabs(npy(a), b) <= (2 * tol if i < 2 else 1e-4) * scale(b), i
