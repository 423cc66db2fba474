"""GPU: the workgroup / item -> (clip, head, ...) decodes that spread the heads of the dense layout over an XCD's L2 channels
(msda_rs.hip, msda_scatter.hip, msda_mfma.hip).  Where a workgroup runs must not change a result, so the risk of a decode is a
(clip, head, part) or (clip, frame, head, band) that nobody owns, or that two own: outputs and gradients start as NaN (run_* of
test_layout_gpu.py) and must come back finite everywhere and equal to the oracle within the suite's tolerances (TOL of
test_layout_gpu.py, nothing of its own).  The cases are the ones the decodes' arithmetic can trip over: 3 clips, so that
workgroup and item counts are not multiples of the 8 XCDs nor of 8 x heads (15 (clip, frame) pairs: 60 / 120 / 240 items for
4 / 8 / 16 heads); 101 queries in 5 frames = 35 tiles per clip, which 3 parts (one tile per wave) and 2 parts (frame split)
do not divide; 4 and 16 heads beside 8; f32 and bf16; every route is forced and asserted through msda_last_route()."""
import functools

import pytest
import torch

from helpers import PYR_A, relayout
from test_layout_gpu import (DTYPES, _env, _mark, _pin, _rounded, check, op_case, op_reference, run_op, run_temporal,
                             temporal_case, temporal_reference_clips)

pytestmark = pytest.mark.gpu

CLIPS, T, LQ = 3, 5, 101
SEEN = set()

ROUTE_SETS = [
    # id, forward label (ROUTES of test_layout_gpu.py), substrings of the backward's route (16-bit types add "grad_value in the
    # storage type" to the labels there), knobs, pins
    ("slab-nt1_gather-slab_owner-level-order", "fwd resident-slab nt1", ("resident-slab kernel, grad_loc/grad_attn", "owner-computes scatter kernel, group-granular"),
     {"MSDA_FWD_RS": "1", "MSDA_FWD_RS_NT": "1", "MSDA_BWD_RS": "1", "MSDA_BWD_RS_FSPLIT": "0", "MSDA_SCATTER_MFMA": "0"},
     {"scatter_order": 1}),
    ("slab-nt2_gather-frame-split_owner-image-order", "fwd resident-slab nt2",
     ("one source frame per workgroup", "owner-computes scatter kernel, group-granular", "image order"),
     {"MSDA_FWD_RS": "1", "MSDA_FWD_RS_NT": "2", "MSDA_BWD_RS": "1", "MSDA_BWD_RS_FSPLIT": "2", "MSDA_SCATTER_MFMA": "0"},
     {"scatter_order": 2}),
    ("slab-nt4_matrix-pipe", "fwd resident-slab nt4", ("matrix-pipe scatter kernel, coarse levels, 2 levels",),
     {"MSDA_FWD_RS": "1", "MSDA_FWD_RS_NT": "4", "MSDA_SCATTER_MFMA": "1"}, {}),
]


@functools.lru_cache(maxsize=None)
def _batch(M, dtype):
    """3 clips of the decoder call with M heads on a layout with gaps, and the oracle of every clip; made once per (M, dtype)."""
    dt = DTYPES[dtype]
    r = _rounded(relayout(temporal_case(300 + M, PYR_A, T=T, W=T - 1, M=M, Lq=LQ, clips=CLIPS), "gaps", 53), dt)
    return r, temporal_reference_clips(r, dt, CLIPS)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("M", [4, 8, 16])
@pytest.mark.parametrize("name,fwd,bwd,env,pins", ROUTE_SETS, ids=[s[0] for s in ROUTE_SETS])
def test_every_clip_and_head_is_owned_once(name, fwd, bwd, env, pins, M, dtype, monkeypatch):
    from devis_amd import _native
    _env(monkeypatch, env)
    dt = DTYPES[dtype]
    r, refs = _batch(M, dtype)
    key = _pin(r, pins, CLIPS) if pins else None
    try:
        got, (rf, rb) = run_temporal(r, dt, clips=CLIPS)
    finally:
        if key:
            _native.pin_route(key, "")
    for c in range(CLIPS):
        check(got, refs[c], r, dt, rows=slice(c * T, (c + 1) * T))
    _mark(fwd, rf, SEEN)
    # (the item order is a pin of the fp32 route key; a 16-bit call keeps the order its own rule picks)
    need = [b for b in bwd if b != "image order" or dtype == "f32"]
    assert all(b in rb for b in need), (need, rb)
    assert ("matrix-pipe" in rb) == (env["MSDA_SCATTER_MFMA"] == "1"), rb


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("M", [4, 8, 16])
def test_the_route_rules_own_choice(M, dtype):
    """The same batches on whatever the route rules pick for them (no knob set)."""
    dt = DTYPES[dtype]
    r, refs = _batch(M, dtype)
    got, _ = run_temporal(r, dt, clips=CLIPS)
    for c in range(CLIPS):
        check(got, refs[c], r, dt, rows=slice(c * T, (c + 1) * T))


@pytest.mark.parametrize("M", [4, 8, 16])
def test_plain_op_three_images(M, monkeypatch):
    """The plain op (one frame per clip): 3 images, 7 tiles each -- 3 x M workgroups on the slab kernels, 3 x M items per band."""
    _env(monkeypatch, {"MSDA_FWD_RS": "1", "MSDA_BWD_RS": "1"})
    r = _rounded(relayout(op_case(400 + M, PYR_A, N=3, M=M, D=32, Lq=LQ), "gaps", 59), torch.float32)
    got, (rf, rb) = run_op(r, torch.float32)
    check(got, op_reference(r, torch.float32), r, torch.float32)
    assert "resident-slab kernel" in rf, rf
    assert "owner-computes scatter kernel" in rb, rb
