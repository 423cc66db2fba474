"""GPU: the owner-computes scatter with five pixels per owner quad and bands of equal height (msda_bwd_value_grp_kernel).

Every case is one fused temporal call -- M = 8, D = 32, 2 frames with a window of 1, 40 queries -- on a single level or a
two-level pyramid, the matrix-pipe scatter switched off so that the owner kernel walks every level, compared with the oracle at
the tolerances tests/test_op_gpu.py uses for this route (fp32: 2e-5 of the largest magnitude; bf16: 1e-2; the float-atomic
"direct" branch: 1e-4).  grad_value and the four sampling gradients start as NaN: whatever a band, a slot or a level does not
write shows.  The band lists the cases name are the ones tests/test_bands_cpu.py checks on the host side.
"""
import numpy as np
import pytest
import torch

from devis_amd.tuning import kSdbgNoFourSlotRule
from helpers import PYR_A, make_temporal_inputs, temporal_reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out")
# top tap rows (h_im = y H - 0.5) put on level 0 of the 45-row cases: both rows of a tap straddle every boundary of the three
# bands of 15 rows (14 | 15, 29 | 30) and of the four bands 12, 11, 11, 11 (11 | 12, 22 | 23, 33 | 34); one tap has its top
# row at -1 (only the bottom row, 0, is inside) and one at 44 (only the top row is inside)
H_IM_45 = (-0.5, 14.4, 29.6, 44.3, 11.5, 22.5, 33.5)


def _round(d, dtype, loc_dtype):
    """The call as the storage types hold it, in float64: value / grad_out through `dtype`, locations and weights through `loc_dtype`."""
    out = {}
    for k, v in d.items():
        if v.dtype.kind != "f":
            out[k] = v
            continue
        t = dtype if k in ("value", "grad_out") else loc_dtype
        out[k] = torch.from_numpy(np.asarray(v, dtype=np.float64)).to(t).double().numpy()
    return out


def _case(seed, shapes, dtype=torch.float32, loc_dtype=None, rows=None, T=2, Lq=40):
    d = make_temporal_inputs(seed, T=T, W=T - 1, M=8, D=32, Lq=Lq, shapes=shapes, Pc=4, Pt=4)
    if rows is not None:
        H = shapes[0][0]
        for i, h_im in enumerate(rows):                 # query i, every head, every point of level 0, both point sets
            y = (h_im + 0.5) / H
            d["loc_c"][:, i, :, 0, :, 1] = y
            d["loc_t"][:, i, :, 0, :, 1] = y            # (window of 1: virtual level 0 is level 0 of the other frame)
    d = _round(d, dtype, loc_dtype or dtype)
    if rows is not None:                                # ... and the rounded coordinates still sit where the case wants them
        H = shapes[0][0]
        for i, h_im in enumerate(rows):
            got = np.floor(d["loc_c"][:, i, :, 0, :, 1].astype(np.float32) * np.float32(H) - np.float32(0.5))
            assert (got == np.floor(h_im)).all(), (h_im, got)
    return d


def _run(d, dtype, loc_dtype=None, gv_dtype=None, clips=1):
    """(out, grad_value, grad_loc_c, grad_aw_c, grad_loc_t, grad_aw_t) as float64 numpy, and the backward's route."""
    from devis_amd import _native
    loc_dtype = loc_dtype or dtype
    t = lambda k, dt: torch.from_numpy(np.ascontiguousarray(d[k])).to(DEV, dt).contiguous()     # noqa: E731
    v, go = t("value", dtype), t("grad_out", dtype)
    lc, ac, lt, at = (t(k, loc_dtype) for k in ("loc_c", "aw_c", "loc_t", "aw_t"))
    shapes, lsi, ftab = (torch.from_numpy(d[k]).to(DEV) for k in ("shapes", "lsi", "ftab"))
    out = torch.full(go.shape, float("nan"), dtype=dtype, device=DEV)
    _native.temporal_forward(v, shapes, lsi, ftab, lc, ac, lt, at, clips, out)
    L, Pc, W, Pt = lc.shape[3], lc.shape[4], ftab.shape[1], lt.shape[4]
    named = _native.grad_value_dtype(v, shapes, lc.shape[1], L, Pc, clips=clips, window=W, Pt=Pt)
    gv = torch.full(v.shape, float("nan"), dtype=gv_dtype or named, device=DEV)
    grads = [torch.full(x.shape, float("nan"), dtype=x.dtype, device=DEV) for x in (lc, ac, lt, at)]
    _native.temporal_backward(v, shapes, lsi, ftab, lc, ac, lt, at, go, clips, gv, *grads)
    torch.cuda.synchronize()
    route = _native.last_route()
    return [x.double().cpu().numpy() for x in [out, gv] + grads], route, named


def _check(got, ref, tol, gv_tol=None):
    names = ("out", "grad_value", "grad_loc_c", "grad_aw_c", "grad_loc_t", "grad_aw_t")
    for n, a, b in zip(names, got, ref):
        assert np.isfinite(a).all(), n                                   # every element written
        err = float(np.abs(a - b).max())
        bound = (gv_tol if n == "grad_value" and gv_tol else tol) * max(1.0, float(np.abs(b).max()))
        print("%s: max error %.3g (bound %.3g)" % (n, err, bound))
        assert err <= bound, (n, err, bound)


@pytest.fixture()
def owner_only(monkeypatch):
    monkeypatch.setenv("MSDA_SCATTER_MFMA", "0")          # every level is the owner kernel's
    # ... with as many slots as its instantiation takes: these calls are a few dozen items, which the planner would keep on four
    monkeypatch.setenv("MSDA_SCATTER_DBG", str(kSdbgNoFourSlotRule))


@pytest.fixture()
def owner_only_planner_choice(monkeypatch):
    monkeypatch.setenv("MSDA_SCATTER_MFMA", "0")


def test_few_item_call_on_the_planner_s_four_slots(owner_only_planner_choice):
    """The same 45 x 80 call as it is planned: 2 x 8 x 3 items are few, so fp32 runs the FOUR-slot instantiation (12, 11, 11, 11)."""
    d = _case(701, [(45, 80)], rows=H_IM_45)
    got, route, _ = _run(d, torch.float32)
    assert "owner-computes scatter kernel, group-granular" in route and "zero-fill" not in route, route
    _check(got, temporal_reference(*(d[k] for k in KEYS)), 2e-5)


FP32_CASES = {
    "45x80: 15, 15, 15": ([(45, 80)], H_IM_45),
    "33x80: 11, 11, 11": ([(33, 80)], (-0.5, 10.5, 21.5, 32.4)),
    "17x80: 9, 8": ([(17, 80)], (-0.5, 8.5, 16.3)),
}


@pytest.mark.parametrize("name", list(FP32_CASES))
def test_balanced_bands_fp32(name, owner_only):
    shapes, rows = FP32_CASES[name]
    d = _case(701, shapes, rows=rows)
    got, route, _ = _run(d, torch.float32)
    assert "owner-computes scatter kernel, group-granular" in route and "zero-fill" not in route and "matrix-pipe" not in route, route
    _check(got, temporal_reference(*(d[k] for k in KEYS)), 2e-5)


def test_a_level_that_became_one_band_leaves_no_records_and_is_fully_overwritten(owner_only):
    """25 x 42 = 1050 pixels: one band of five slots (two of four), so the gather pass leaves no culling records for it and the
    owner kernel takes every group as a candidate; with the 13 x 21 level beside it.  grad_value starts as NaN."""
    shapes = [(25, 42), (13, 21)]
    d = _case(702, shapes, rows=(-0.5, 11.5, 12.5, 24.3))
    got, route, _ = _run(d, torch.float32)
    assert "owner-computes scatter kernel, group-granular" in route and "zero-fill" not in route, route
    _check(got, temporal_reference(*(d[k] for k in KEYS)), 2e-5)


@pytest.mark.parametrize("loc_dtype", [torch.bfloat16, torch.float32], ids=["bf16_locations", "fp32_locations"])
def test_five_and_four_slot_instantiations_side_by_side_bf16(loc_dtype, owner_only):
    """The planner's per-call band size: a bf16 call whose grad_value is written in bf16 runs the five-slot instantiation (45 x
    80: three bands), the same call with a float grad_value the four-slot one (four bands: 12, 11, 11, 11) -- with bf16 and
    with fp32 sampling locations.  Both against the oracle, and against each other within one bf16 unit in the last place."""
    d = _case(703, [(45, 80)], torch.bfloat16, loc_dtype, rows=H_IM_45)
    ref = temporal_reference(*(d[k] for k in KEYS))
    five, r5, named = _run(d, torch.bfloat16, loc_dtype)
    assert named == torch.bfloat16 and "grad_value in the storage type" in r5, r5
    four, r4, _ = _run(d, torch.bfloat16, loc_dtype, gv_dtype=torch.float32)
    assert "owner-computes scatter kernel, group-granular" in r4 and "storage type" not in r4, r4
    _check(five, ref, 1e-2)
    _check(four, ref, 1e-2)
    a, b = four[1], five[1]
    assert float((np.abs(a - b) - 2.0 ** -7 * np.abs(a)).max()) <= 1e-6
    for x, y in zip(five[2:], four[2:]):                   # the gather pass does not depend on the scatter's bands
        assert np.array_equal(x, y)


def test_direct_branch_of_a_row_wider_than_a_band_is_unchanged(owner_only):
    """3 x 1300: a row wider than 1024 pixels (and than the 1280 of a five-slot band) -- float atomics into a grad_value
    zero-filled by its own launch, in every instantiation as before."""
    d = _case(704, [(3, 1300)], rows=(-0.5, 0.5, 2.3))
    got, route, _ = _run(d, torch.float32)
    assert "owner-computes scatter kernel, group-granular" in route and "zero-fill of pixels outside the bands" in route, route
    _check(got, temporal_reference(*(d[k] for k in KEYS)), 2e-5, gv_tol=1e-4)        # (float atomics: as test_op_gpu's wide level)


def test_decoder_call_on_the_automatic_route():
    """The 360x640 pyramid, 2 clips of 6 frames, 300 queries: whatever route the rules pick, clip by clip against the oracle."""
    clips, T = 2, 6
    ds = [_case(710 + c, PYR_A, T=T, Lq=300) for c in range(clips)]
    cat = {k: (np.concatenate([x[k] for x in ds], 0) if k not in ("shapes", "lsi", "ftab") else ds[0][k]) for k in ds[0]}
    got, route, _ = _run(cat, torch.float32, clips=clips)
    assert "owner-computes scatter kernel, group-granular" in route, route
    for c, d in enumerate(ds):
        ref = list(temporal_reference(*(d[k] for k in KEYS)))
        # grad_loc is discontinuous where a pixel coordinate crosses an integer, and among 2 x 6 x 300 x 8 x 96 points some lie
        # within one fp32 unit of a cell border: the location gradients are compared with the oracle evaluated in the SAME (fp32)
        # arithmetic, whose x W - 0.5 rounding the kernels reproduce bit for bit (as test_op_gpu's full-size decoder call does);
        # out, grad_value and the weight gradients are continuous there and stay against the float64 oracle
        ref32 = temporal_reference(*(d[k].astype(np.float32) if d[k].dtype.kind == "f" else d[k] for k in KEYS))
        ref[2], ref[4] = ref32[2].astype(np.float64), ref32[4].astype(np.float64)
        _check([g[c * T:(c + 1) * T] for g in got], ref, 2e-5)
