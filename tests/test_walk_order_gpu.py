"""GPU: the resident-slab gather pass with its workgroups taken first to last and last to first (MSDA_WALK = 0 / 1,
GatherPlan::walk_down in csrc/msda_plan.hip; the kernel's decode in csrc/msda_rs.hip).  The order is speed only, so both must give
the oracle's gradients, the same bits of grad_loc / grad_attn as each other, and write every element of every gradient.

Shapes: the small pyramid of tests/test_layout_gpu.py, 17 clips (no multiple of the 8 XCDs: the runs of the XCDs differ in length
and do not end on clip boundaries), 20 queries (no multiple of a 16-row tile), 8 (or 5) heads of 32 channels -- 85 to 816 workgroups, ten to a hundred per
XCD, so first, middle and last workgroups of a run are all decoded both ways.  T = 3 frames with both grids of
the kernel ((clip, head, part) walking the frames, and one source frame per workgroup), and T = 1 without a window (the plain op).
fp32 takes the forward's alternating head order when it walks down, bf16 and five heads the plain one.  Every gradient buffer starts
as NaN (run_op / run_temporal of tests/test_layout_gpu.py), so an element no workgroup wrote is not finite."""
import functools

import numpy as np
import pytest
import torch

from test_layout_gpu import SMALL, TOL, _env, _rounded, op_case, op_reference, run_op, run_temporal, temporal_case, temporal_reference_clips
from test_op_gpu import _maxabs

pytestmark = pytest.mark.gpu

CLIPS, LQ = 17, 20
DOWN = "last workgroup first"
GRIDS = {       # knobs, what msda_last_route() must say of the backward
    "frames walked": ({"MSDA_BWD_RS": "1", "MSDA_BWD_RS_FSPLIT": "0"}, "msda backward (resident-slab kernel, grad_loc/grad_attn)"),
    "frame per workgroup": ({"MSDA_BWD_RS": "1", "MSDA_BWD_RS_FSPLIT": "2"}, "grad_loc/grad_attn, one source frame per workgroup)"),
}


@functools.lru_cache(maxsize=None)
def _temporal(dtype, M):
    """The 17-clip call of T = 3 frames (window: the other two) rounded to `dtype`, and the oracle's results per clip: made once."""
    r = _rounded(temporal_case(900 + M, SMALL, T=3, W=2, M=M, D=32, Lq=LQ, clips=CLIPS), dtype)
    r["gap"] = np.zeros(r["value"].shape[1], bool)
    return r, temporal_reference_clips(r, dtype, clips=CLIPS)


@functools.lru_cache(maxsize=None)
def _plain():
    """17 single frames without a window: the plain op, N = 17."""
    r = _rounded(op_case(917, SMALL, N=CLIPS, M=8, D=32, Lq=LQ), torch.float32)
    r["gap"] = np.zeros(r["value"].shape[1], bool)
    return r, op_reference(r, torch.float32)


def _both_directions(run, label, monkeypatch):
    got = {}
    for walk in ("0", "1"):
        monkeypatch.setenv("MSDA_WALK", walk)
        got[walk], (_, rb) = run()
        assert label in rb and (DOWN in rb) == (walk == "1"), (walk, rb)
    return got["0"], got["1"]


def _check(up, down, ref, dtype):
    """`ref`: the oracle's (out, grad_value, gradients of the points ...) for the whole batch."""
    tf, tb = TOL[dtype]
    for name, got in (("up", up), ("down", down)):
        for i, (a, b) in enumerate(zip(got, ref)):
            assert np.isfinite(a).all(), (name, i, "an element was not written")
            err, scale = _maxabs(a, b), max(1.0, float(np.abs(b).max()))
            assert err <= (tf if i == 0 else tb) * scale, (name, i, err, scale)
    for i, (a, b) in enumerate(zip(up, down)):
        if i == 1:          # grad_value: the scatter's fp32 sums follow its work tickets, not the gather pass -- equal to the oracle's tolerance
            assert _maxabs(a, b) <= TOL[dtype][1] * max(1.0, float(np.abs(ref[1]).max())), _maxabs(a, b)
        else:               # the forward and the gather pass: the same workgroup computes the same sums in the same order
            assert np.array_equal(a, b), (i, _maxabs(a, b))


@pytest.mark.parametrize("dtype,M", [(torch.float32, 8), (torch.bfloat16, 8), (torch.float32, 5)], ids=["f32", "bf16", "f32-5heads"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_temporal_gather_pass_in_both_directions(grid, dtype, M, monkeypatch):
    env, label = GRIDS[grid]
    _env(monkeypatch, env)
    r, refs = _temporal(dtype, M)
    up, down = _both_directions(lambda: run_temporal(r, dtype, clips=CLIPS), label, monkeypatch)
    ref = [np.concatenate([c[i] for c in refs], 0) for i in range(6)]
    _check(up, down, ref, dtype)


def test_single_frame_gather_pass_in_both_directions(monkeypatch):
    _env(monkeypatch, {"MSDA_BWD_RS": "1"})
    r, ref = _plain()
    up, down = _both_directions(lambda: run_op(r, torch.float32), GRIDS["frames walked"][1], monkeypatch)
    _check(up, down, ref, torch.float32)


def test_rule_keeps_small_calls_first_to_last(monkeypatch):
    """Without the knob the planner decides from the call's size: these calls are a few MB."""
    monkeypatch.delenv("MSDA_WALK", raising=False)
    _env(monkeypatch, GRIDS["frame per workgroup"][0])
    r, _ = _temporal(torch.float32, 8)
    _, (_, rb) = run_temporal(r, torch.float32, clips=CLIPS)
    assert GRIDS["frame per workgroup"][1] in rb and DOWN not in rb, rb
