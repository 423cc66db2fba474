"""Pins the CPU oracle (oracle/) to the golden vectors made from the reference's own Python oracle
``ms_deform_attn_core_pytorch`` + autograd (tests/golden/make_golden.py).  CPU only.

The reference ships no numeric known-answer vectors for this path (src/models/ops/test.py only
prints allclose/gradcheck verdicts), so these fixtures -- outputs of the reference itself, generated
in the build container -- are the pin."""
import numpy as np
import pytest
import torch

from conftest import OP_FIXTURES, golden


@pytest.mark.parametrize("name", OP_FIXTURES)
def test_c_oracle_forward_fp64_matches_reference(oracle, name):
    g = golden(name)
    out = oracle.forward(g["value"].astype(np.float64), g["spatial_shapes"], g["level_start_index"],
                         g["sampling_locations"].astype(np.float64),
                         g["attention_weights"].astype(np.float64))
    # reference test.py:40 uses torch.allclose defaults (rtol 1e-5, atol 1e-8) in fp64; we are far tighter
    np.testing.assert_allclose(out, g["out"], rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("name", OP_FIXTURES)
def test_c_oracle_backward_fp64_matches_reference_autograd(oracle, name):
    g = golden(name)
    gv, gl, ga = oracle.backward(g["value"].astype(np.float64), g["spatial_shapes"],
                                 g["level_start_index"], g["sampling_locations"].astype(np.float64),
                                 g["attention_weights"].astype(np.float64), g["grad_output"])
    np.testing.assert_allclose(gv, g["grad_value"], rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(ga, g["grad_attn_weight"], rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(gl, g["grad_sampling_loc"], rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("name", OP_FIXTURES)
def test_c_oracle_forward_fp32(oracle, name):
    g = golden(name)
    out = oracle.forward(g["value"], g["spatial_shapes"], g["level_start_index"],
                         g["sampling_locations"], g["attention_weights"])
    assert out.dtype == np.float32
    # BASELINE.json: <= 1e-4 max abs in fp32 (reference test.py:56 only asks rtol 1e-2 / atol 1e-3)
    assert np.abs(out - g["out"]).max() <= 1e-6
    assert np.abs(out - g["out_f32"]).max() <= 1e-6


@pytest.mark.parametrize("name", OP_FIXTURES)
def test_torch_restatement_matches_reference(oracle, name):
    """oracle.grid_sample_forward is what bench.py times as the CPU baseline."""
    g = golden(name)
    v, l, a = (torch.from_numpy(g[k].astype(np.float64)).requires_grad_(True)
               for k in ("value", "sampling_locations", "attention_weights"))
    out = oracle.grid_sample_forward(v, torch.from_numpy(g["spatial_shapes"]), l, a)
    np.testing.assert_allclose(out.detach().numpy(), g["out"], rtol=1e-12, atol=1e-15)
    gv, gl, ga = torch.autograd.grad(out, (v, l, a), torch.from_numpy(g["grad_output"]))
    np.testing.assert_allclose(gv.numpy(), g["grad_value"], rtol=1e-11, atol=1e-14)
    # exactly on h_im == -1 / w_im == -1 grid_sample differentiates one-sidedly while the reference
    # CUDA kernel skips the point (cuh:288); the golden follows the kernel (see make_golden.py)
    keep = ~g["on_minus_one_edge"][..., None]
    np.testing.assert_allclose(gl.numpy() * keep, g["grad_sampling_loc"], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(ga.numpy(), g["grad_attn_weight"], rtol=1e-11, atol=1e-14)


def test_reference_testpy_procedure(oracle):
    """The reference's own check (src/models/ops/test.py:30-58), restated with asserts: forward fp64
    allclose at torch defaults, forward fp32 at rtol 1e-2 / atol 1e-3, on its shapes and seed."""
    g = golden("op_testpy_shape")
    assert g["value"].shape == (1, 30, 2, 2) and g["sampling_locations"].shape == (1, 2, 2, 2, 2, 2)
    o64 = oracle.forward(g["value"].astype(np.float64), g["spatial_shapes"], g["level_start_index"],
                         g["sampling_locations"].astype(np.float64),
                         g["attention_weights"].astype(np.float64))
    assert np.allclose(o64, g["out"], rtol=1e-5, atol=1e-8)
    o32 = oracle.forward(g["value"], g["spatial_shapes"], g["level_start_index"],
                         g["sampling_locations"], g["attention_weights"])
    assert np.allclose(o32, g["out_f32"], rtol=1e-2, atol=1e-3)


def test_skipped_points_have_zero_gradients(oracle):
    """cuh:288 + zero-filled grads (ms_deform_attn_cuda.cu:121-123)."""
    g = golden("op_out_of_range")
    H, W = g["spatial_shapes"][0]
    loc = g["sampling_locations"].astype(np.float64)
    y = loc[0, :, 0, 0, 0, 1] * H - 0.5
    outside = ~((y > -1) & (y < H))
    assert outside.sum() >= 4            # the fixture really contains skipped points
    assert np.all(g["grad_attn_weight"][0, outside, 0, 0, 0] == 0)
    assert np.all(g["grad_sampling_loc"][0, outside, 0, 0, 0] == 0)


# ---- level layouts that do not tile [0, S) (include/msda.h): the oracle the GPU layout tests compare against --------------------
from helpers import (LAYOUTS, PYR_A, gaps_zeroed, level_rows, make_inputs, make_temporal_inputs, relayout,  # noqa: E402
                     temporal_reference, window_level_starts)

_TKEYS = ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", LAYOUTS)
def test_oracle_is_layout_independent(oracle, kind, dtype):
    """Same call, level rows moved (gaps, 64-row alignment, reordered levels): forward, grad_loc and grad_attn bit-identical,
    the level rows of grad_value bit-identical, its gap rows exactly 0 -- with the gaps zeroed and with them NaN (never read)."""
    d = make_inputs(41, 2, 3, 8, 29, [(9, 11), (6, 10), (4, 5), (2, 3)], 4, "wide", dtype, value_scale=1.0)
    r = relayout(d, kind, 7)
    assert r["gap"].any() and r["value"].shape[1] > d["value"].shape[1]
    base = [oracle.forward(d["value"], d["shapes"], d["lsi"], d["loc"], d["aw"])]
    base += oracle.backward(d["value"], d["shapes"], d["lsi"], d["loc"], d["aw"], d["grad_out"])
    for x in (gaps_zeroed(r), r):
        got = [oracle.forward(x["value"], x["shapes"], x["lsi"], x["loc"], x["aw"])]
        got += oracle.backward(x["value"], x["shapes"], x["lsi"], x["loc"], x["aw"], x["grad_out"])
        for i in (0, 2, 3):
            assert np.array_equal(got[i], base[i]), i
        assert np.array_equal(level_rows(got[1], x), base[1])
        assert (got[1][:, x["gap"]] == 0).all()


@pytest.mark.parametrize("kind", LAYOUTS)
def test_temporal_reference_is_layout_independent(kind):
    """The fused temporal op's oracle on a relaid clip: the same layout in every frame, the window's stacked value at lsi + w * S."""
    ftab = np.array([[1, 1], [0, 2], [1, 3], [3, 0]], dtype=np.int32)        # repeated frames
    d = make_temporal_inputs(43, 4, 2, 2, 8, 17, [(7, 9), (5, 6), (3, 4)], 3, 2, ftab=ftab, dtype=np.float64)
    r = relayout(d, kind, 11)
    base = temporal_reference(*(d[k] for k in _TKEYS))
    got = temporal_reference(*(gaps_zeroed(r)[k] for k in _TKEYS))
    for i in (0, 2, 3, 4, 5):
        assert np.array_equal(got[i], base[i]), i
    assert np.array_equal(level_rows(got[1], r), base[1])
    assert (got[1][:, r["gap"]] == 0).all()


@pytest.mark.parametrize("shapes", [PYR_A, [(7, 9), (5, 6), (3, 4)], [(4, 4)]])
@pytest.mark.parametrize("W", [1, 2, 5])
def test_window_level_starts_equal_the_cumsum_on_compact_layouts(oracle, shapes, W):
    """For a compact pyramid the generalised window layout is the reference's spatial_shapes.repeat(window) cumsum."""
    shapes = np.asarray(shapes, dtype=np.int64)
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    assert np.array_equal(window_level_starts(oracle.level_start_index(shapes), S, W),
                          oracle.level_start_index(np.tile(shapes, (W, 1))))


@pytest.mark.parametrize("kind", LAYOUTS)
def test_relayout_keeps_every_level_row_and_poisons_the_rest(kind):
    d = make_inputs(3, 2, 2, 4, 5, PYR_A, 2, dtype=np.float32)
    r = relayout(d, kind, 5)
    shapes, lsi = r["shapes"], r["lsi"]
    hw = shapes[:, 0] * shapes[:, 1]
    assert np.array_equal(level_rows(r["value"], r), d["value"])
    assert np.isnan(r["value"][:, r["gap"]]).all() and r["gap"].sum() == r["value"].shape[1] - hw.sum()
    ends = sorted(zip(lsi.tolist(), (lsi + hw).tolist()))
    assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:]))                 # no level overlaps another
    if kind in ("gaps", "reversed"):
        assert lsi.min() > 0 and lsi.max() + hw[lsi.argmax()] < r["value"].shape[1]
    if kind == "aligned":
        assert (lsi % 64 == 0).all()
    if kind == "tail_gap":
        assert lsi[-1] - (lsi[-2] + hw[-2]) >= hw[-1] and np.array_equal(lsi[:-1], d["lsi"][:-1])
    if kind == "reversed":
        assert (np.diff(lsi) < 0).all()
