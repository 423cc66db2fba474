"""CPU tests of the run-length encoder: the numpy oracle against itself and hand-written cases, the C ABI of
include/maskrle.h (exports, version, argument errors, workspace arithmetic -- no compute calls), the host code (shape checks,
errors, fake tensors, export), the tracker wiring with ``gpu_rle=True`` on a fake operator, and the committed resource table.
The kernels themselves are tests/test_maskrle_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import maskiou_oracle as O
import maskrle_oracle as R
from conftest import ROOT
from test_maskiou_cpu import StandInMaskUtil, fake_binarize, reference_choice, stand_in_modules


# ---- oracle ----------------------------------------------------------------------------------------------------------

def test_oracle_on_hand_written_cases():
    assert R.runs_of(np.zeros((3, 4), bool)) == [12]
    assert R.runs_of(np.ones((3, 4), bool)) == [0, 12]
    assert R.runs_of(np.eye(3, 4)) == [0, 1, 3, 1, 3, 1, 3]
    col = np.zeros((3, 4), bool)
    col[:, 1] = True                    # one column is one run of the column-major walk
    assert R.runs_of(col) == [3, 3, 6]
    row = np.zeros((3, 4), bool)
    row[1, :] = True                    # one row is a run per column
    assert R.runs_of(row) == [1, 1, 2, 1, 2, 1, 2, 1, 1]
    assert all(isinstance(c, int) for c in R.runs_of(row))


@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (9, 1), (5, 7), (16, 4), (67, 13)])
def test_oracle_decode_inverts_runs_of(H, W):
    g = np.random.default_rng(H * 100 + W)
    yy, xx = np.mgrid[:H, :W]
    for bits in (g.random((H, W)) < 0.5, g.random((H, W)) < 0.05, np.zeros((H, W), bool), np.ones((H, W), bool),
                 (yy + xx) % 2 == 0, (yy + xx) % 2 == 1):
        counts = R.runs_of(bits)
        assert sum(counts) == H * W and all(c > 0 for c in counts[1:])
        assert np.array_equal(R.decode(counts, H, W), bits)
        assert (counts[0] == 0) == bool(bits[0, 0])
    if H % 2:           # an odd column keeps the checkerboard alternating across columns: the most runs a mask can have
        assert len(R.runs_of((yy + xx) % 2 == 0)) == H * W + 1 and len(R.runs_of((yy + xx) % 2 == 1)) == H * W


# ---- library ---------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_maskrle_h_declares_and_versions_agree():
    from devis_amd import _maskiou, _maskrle, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "maskrle.h")).read()
    declared = set(re.findall(r"\b(maskrle_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_maskrle.EXPORTED_SYMBOLS) and len(declared) == 5
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _maskrle.load()
    assert lib.maskrle_version() == _maskrle.MASKRLE_ABI_VERSION == int(re.search(r"#define MASKRLE_ABI_VERSION (\d+)", header).group(1))
    names = ("BITS_PIXELS", "WORD_PIXELS", "BITS_SRC", "RUNS_THREADS")
    tiles = tuple(int(re.search(r"#define MASKRLE_TILE_%s (\d+)" % n, header).group(1)) for n in names)
    assert tiles == (_maskrle.TILE_BITS_PIXELS, _maskrle.TILE_WORD_PIXELS, _maskrle.TILE_BITS_SRC, _maskrle.TILE_RUNS_THREADS)
    assert all(_maskrle.tile(t) > 0 for t in tiles) and lib.maskrle_tile(9) == -1
    assert _maskrle.tile(_maskrle.TILE_WORD_PIXELS) == 64
    assert _maskrle.tile(_maskrle.TILE_BITS_PIXELS) % _maskrle.tile(_maskrle.TILE_WORD_PIXELS) == 0
    assert dict(re.findall(r"MASKRLE_(F32|F64|BF16|F16) = (\d)", header)) == {"F32": "0", "F64": "1", "BF16": "2", "F16": "3"}
    # the header states the runs and the row layout, names whose bits they are, and refers to the tap rule without restating it
    for phrase in ("column-major", "starting with a run of zeros", "runs[n, 0]", "maskiou_binarize", "rule of maskloss.h"):
        assert phrase in header, phrase
    assert "max(scale" not in header and "0.5" not in header
    assert os.path.join(build.include_dir(), "maskrle.h") in build._headers()
    assert any(s.endswith("maskrle.hip") for s in build.sources())
    assert "maskrle.h" in open(os.path.join(ROOT, "setup.py")).read() and "maskrle.h" in build.include_dir.__doc__
    # maskiou.h is as it was: six symbols, version 1
    iou = open(os.path.join(ROOT, "include", "maskiou.h")).read()
    assert len(set(re.findall(r"\b(maskiou_[a-z_0-9]+)\s*\(", iou))) == 6 == len(_maskiou.EXPORTED_SYMBOLS)
    assert "#define MASKIOU_ABI_VERSION 1\n" in iou and _maskiou.load().maskiou_version() == 1


def test_the_tap_rule_has_one_definition():
    csrc = os.path.join(ROOT, "devis_amd", "csrc")
    text = {name: open(os.path.join(csrc, name)).read() for name in ("maskiou.hip", "maskrle.hip", "mask_taps.h")}
    for name in ("maskiou.hip", "maskrle.hip"):
        assert '#include "mask_taps.h"' in text[name]
        assert "Tap<A> tap_at(" not in text[name] and " A lerp_of(" not in text[name] and "struct Tap" not in text[name]
    assert "Tap<A> tap_at(" in text["mask_taps.h"] and " A lerp_of(" in text["mask_taps.h"] and "logit_at(" in text["mask_taps.h"]


def test_maskrle_argument_errors_without_gpu():
    from devis_amd import _maskrle
    lib = _maskrle.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.maskrle_last_error

    def encode(dtype=0, src=p, N=3, h=12, w=20, H=45, W=80, max_runs=641, ws=p, runs=p):
        return lib.maskrle_encode(dtype, src, N, h, w, H, W, max_runs, ws, runs, None)

    for dtype in (9, -1, 4):
        assert encode(dtype=dtype) == -1 and b"dtype" in err()
    for bad in (dict(h=0), dict(H=0), dict(w=-2), dict(W=0), dict(h=-1), dict(H=-7), dict(N=-1)):
        assert encode(**bad) == -1 and b"positive" in err(), bad
    assert encode(H=65536, W=65536) == -1 and b"31 bits" in err()
    assert encode(H=32768, W=65536) == -1 and b"31 bits" in err()           # 2^31 itself
    assert encode(h=65536, w=65536) == -1 and b"31 bits" in err()
    for bad in (0, -1, -(2 ** 31)):
        assert encode(max_runs=bad) == -1 and b"max_runs" in err(), bad
    for name in ("src", "ws", "runs"):
        assert encode(**{name: None}) == -1 and b"null pointer" in err(), name
    assert encode(N=0, src=None, ws=None, runs=None) == 0 and err() == b""          # nothing launched, nothing dereferenced
    assert encode(N=0, max_runs=0) == -1                                             # (checked before the no-op)


def test_workspace_arithmetic():
    from devis_amd import _maskrle
    lib = _maskrle.load()
    word = _maskrle.tile(_maskrle.TILE_WORD_PIXELS)
    up = lambda n: (n + 255) // 256 * 256      # noqa: E731
    for N, H, W in ((1, 1, 1), (1, 8, 8), (3, 5, 13), (7, 67, 61), (100, 720, 1280), (1, 32767, 65536), (2, 1, 2 ** 31 - 1)):
        got = lib.maskrle_workspace_bytes(N, H, W)
        assert got == up(N * -(-H * W // word) * 8) and got % 256 == 0 and got > 0, (N, H, W)
    assert lib.maskrle_workspace_bytes(0, 720, 1280) == 0
    for N in (1, 8, 100):
        assert lib.maskrle_workspace_bytes(N, 720, 1280) < N * 720 * 1280
        assert lib.maskrle_workspace_bytes(N, 720, 1280) <= N * 720 * 1280 // 8 + 256
    for bad in ((-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, -4, 4), (1, 65536, 65536), (1, 32768, 65536)):
        assert lib.maskrle_workspace_bytes(*bad) == -1, bad
    with pytest.raises(RuntimeError, match="31 bits"):
        _maskrle.workspace_bytes(1, 65536, 65536)


def test_the_resource_table_shows_no_scratch_in_any_instantiation():
    lines = [ln for ln in open(os.path.join(ROOT, "profiles", "maskrle_resource_usage.txt")) if not ln.startswith("#")]
    kernels = {}
    for ln in lines:
        name, rest = ln.split(":", 1)
        kernels[name] = rest
        assert " 0 VGPR spills, 0 SGPR spills, 0 scratch," in rest, ln
    for kernel, count in (("bits_kernel", 4), ("runs_kernel", 1)):
        assert sum(kernel in k for k in kernels) == count, kernel
    assert len(kernels) == 5


# ---- host ------------------------------------------------------------------------------------------------------------

def test_operator_raises_on_cpu_tensors_and_on_bad_arguments_before_any_launch(monkeypatch):
    import devis_amd
    from devis_amd import _maskrle
    from devis_amd.functions import mask_rle as M

    def no_launch(*a, **k):
        raise AssertionError("a kernel call was made")

    monkeypatch.setattr(_maskrle, "encode", no_launch)
    src = torch.zeros(3, 6, 10)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.mask_run_lengths(src, (24, 40))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.mask_run_lengths(src[:0], (24, 40))
    with pytest.raises(RuntimeError, match="src must be \\[N, h, w\\]"):
        devis_amd.mask_run_lengths(src[0], (24, 40))
    with pytest.raises(RuntimeError, match="size must be"):
        devis_amd.mask_run_lengths(src, (24, 40, 2))
    with pytest.raises(RuntimeError, match="is empty"):
        devis_amd.mask_run_lengths(src, (24, 0))
    with pytest.raises(RuntimeError, match="31 bits"):
        devis_amd.mask_run_lengths(src, (65536, 65536), max_runs=10)
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        devis_amd.mask_run_lengths(src.to(torch.int32), (24, 40))
    for bad in (0, -1):
        with pytest.raises(ValueError, match="max_runs"):
            devis_amd.mask_run_lengths(src, (24, 40), max_runs=bad)
    with pytest.raises(RuntimeError, match="mask_run_lengths: src requires a gradient"):
        devis_amd.mask_run_lengths(src.clone().requires_grad_(True), (24, 40))
    with torch.no_grad(), pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.mask_run_lengths(src.clone().requires_grad_(True), (24, 40))         # under no_grad the flag is no objection
    assert "mask_run_lengths" in devis_amd.__all__ and devis_amd.mask_run_lengths is devis_amd.ops.mask_run_lengths

    meta = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="meta")      # noqa: E731
    assert M.check_src(meta(3, 6, 10), (24, 40), 5) == (3, 6, 10, 24, 40, 5)
    assert M.check_src(meta(0, 6, 10, dtype=torch.bfloat16), [5, 5], 1)[0] == 0
    with pytest.raises(RuntimeError, match="would be empty"):
        M.check_src(meta(3, 6, 0), (24, 40), 5)
    with pytest.raises(RuntimeError, match="would be empty"):
        M.check_src(meta(3, 0, 6), (24, 40), 5)
    # the default cap: every pixel a run of its own where that is less than eight runs per column
    assert M.default_max_runs(720, 1280) == 8 * 1280 + 1 and M.default_max_runs(45, 80) == 641
    assert M.default_max_runs(8, 5) == 41 and M.default_max_runs(7, 5) == 36 and M.default_max_runs(1, 1) == 2
    assert M.default_max_runs(3, 1000) == 3001


def _nodes(graph, name):
    return [n for n in graph.nodes if n.op == "call_function" and name in str(n.target)]


def test_fake_tensors_know_the_shape_from_n_size_and_max_runs():
    from torch.fx.experimental.proxy_tensor import make_fx
    from devis_amd import ops
    meta = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")      # noqa: E731
    for dtype in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
        for size, max_runs, cols in (([45, 80], 641, 642), ([45, 80], 7, 8), ([3, 2], 1, 2)):
            gm = make_fx(lambda s: ops.mask_run_lengths_op(s, size, max_runs), tracing_mode="fake")(meta(5, 12, 20, dtype=dtype))      # noqa: B023
            nodes = _nodes(gm.graph, "mask_run_lengths")
            assert len(nodes) == 1
            val = nodes[0].meta["val"]
            assert tuple(val.shape) == (5, cols) and val.dtype == torch.int32 and val.is_contiguous()
    gm = make_fx(lambda s: ops.mask_run_lengths_op(s, [45, 80], 3), tracing_mode="fake")(meta(0, 12, 20))
    assert tuple(_nodes(gm.graph, "mask_run_lengths")[0].meta["val"].shape) == (0, 4)
    with pytest.raises(Exception, match="max_runs"):
        make_fx(lambda s: ops.mask_run_lengths_op(s, [45, 80], 0), tracing_mode="fake")(meta(5, 12, 20))
    with pytest.raises(Exception, match="src must be"):
        make_fx(lambda s: ops.mask_run_lengths_op(s, [45, 80], 5), tracing_mode="fake")(meta(5, 2, 12, 20))


@pytest.mark.parametrize("dynamic", [False, True])
def test_export_gives_one_op_node_for_static_and_dynamic_sizes(dynamic):
    import devis_amd

    class Runs(torch.nn.Module):
        def forward(self, src):
            return devis_amd.mask_run_lengths(src, (45, 80)), devis_amd.mask_run_lengths(src, (45, 80), max_runs=9)

    D = torch.export.Dim
    shapes = ({0: D("N", min=2, max=512), 1: D("h", min=2, max=512), 2: D("w", min=2, max=512)},) if dynamic else None
    ep = torch.export.export(Runs(), (torch.empty(5, 12, 20, device="meta"),), dynamic_shapes=shapes)
    nodes = _nodes(ep.graph, "mask_run_lengths")
    assert len(nodes) == 2
    for node, cols in zip(nodes, (642, 10)):
        val = node.meta["val"]
        assert val.shape[1] == cols and val.dtype == torch.int32
        assert isinstance(val.shape[0], int) != dynamic


# ---- the tracker wiring with gpu_rle=True ---------------------------------------------------------------------------------

class StandInRleUtil(StandInMaskUtil):
    """Records what it is asked to pack, and what it is asked to encode."""

    def __init__(self):
        super().__init__()
        self.packed = []

    def frPyObjects(self, obj, h, w):
        self.packed.append((obj, h, w))
        return {"size": [h, w], "counts": b"packed%d" % len(self.packed)}


def fake_run_lengths(calls):
    """``ops.mask_run_lengths`` by the numpy oracle on torch's own upsample."""
    def mask_run_lengths(src, size, *, max_runs=None):
        H, W = size
        max_runs = min(H * W + 1, 8 * W + 1) if max_runs is None else max_runs
        calls.append((tuple(src.shape), tuple(size), max_runs))
        bits = F.interpolate(src[:, None].float(), size=tuple(size), mode="bilinear", align_corners=False)[:, 0] > 0
        rows = torch.zeros(src.shape[0], 1 + max_runs, dtype=torch.int32)
        for n in range(src.shape[0]):
            counts = R.runs_of(bits[n].numpy())
            rows[n, 0] = len(counts)
            keep = counts[:max_runs]
            rows[n, 1:1 + len(keep)] = torch.tensor(keep, dtype=torch.int32)
        return rows
    return mask_run_lengths


def rle_modules(**kw):
    tm, mm, tracker = stand_in_modules(**kw)
    tm.mask_util = StandInRleUtil()
    return tm, mm, tracker


@pytest.mark.parametrize("binary", [False, True])
def test_process_masks_with_gpu_rle_packs_the_counts_and_encodes_nothing(binary, monkeypatch):
    import devis_amd
    from devis_amd import ops
    calls, byte_calls = [], []
    monkeypatch.setattr(ops, "mask_run_lengths", fake_run_lengths(calls))
    monkeypatch.setattr(ops, "binarize_masks", fake_binarize(byte_calls))
    tm, mm, tracker = rle_modules(overlap=2, use_binary_mask_iou=binary)
    previous = devis_amd.patch_tracker(tm, mm, gpu_rle=True)
    masks = O.blob_logits(6, 1, 5, 7, 3)[:, 0].float()
    want = F.interpolate(masks[:, None], size=(15, 21), mode="bilinear", align_corners=False)[:, 0] > 0
    for start_idx, idx in ((0, 0), (0, 1), (1, 2), (3, 1)):
        calls.clear()
        tm.mask_util.packed.clear()
        out = tracker.process_masks(start_idx, idx, (15, 21), masks)
        choice = reference_choice(binary, 2, start_idx, idx, 6)
        assert [isinstance(m, dict) for m in out] == choice
        assert [isinstance(m, devis_amd.LogitMask) for m in out] == [not c for c in choice]
        assert calls == ([((sum(choice), 5, 7), (15, 21), 8 * 21 + 1)] if any(choice) else [])      # one operator call
        assert tm.mask_util.seen == [] and byte_calls == []                                            # no encode, no bytes
        assert len(tm.mask_util.packed) == sum(choice)
        k = 0
        for t, m in enumerate(out):
            if not choice[t]:
                assert torch.equal(m.logits, masks[t]) and m.size == (15, 21)
                continue
            obj, h, w = tm.mask_util.packed[k]
            k += 1
            assert (h, w) == (15, 21) and obj["size"] == [15, 21] and set(obj) == {"size", "counts"}
            assert type(obj["counts"]) is list and all(type(c) is int for c in obj["counts"])
            assert np.array_equal(R.decode(obj["counts"], 15, 21), want[t].numpy())
            assert m["counts"] == "packed%d" % k and isinstance(m["counts"], str) and m["size"] == [15, 21]
    devis_amd.unpatch_tracker(tm, mm, previous)
    assert tracker.process_masks(0, 0, (15, 21), masks) == "theirs"


def test_a_mask_over_the_cap_takes_the_byte_path_alone_and_the_order_is_kept(monkeypatch):
    from devis_amd import ops, tracking
    calls, byte_calls = [], []
    monkeypatch.setattr(ops, "mask_run_lengths", fake_run_lengths(calls))
    monkeypatch.setattr(ops, "binarize_masks", fake_binarize(byte_calls))
    util = StandInRleUtil()
    masks = O.blob_logits(5, 1, 5, 7, 7)[:, 0].float()
    g = torch.Generator().manual_seed(5)
    masks[1] = torch.randn(5, 7, generator=g)           # noise: many runs
    masks[3] = torch.randn(5, 7, generator=g)
    want = F.interpolate(masks[:, None], size=(15, 21), mode="bilinear", align_corners=False)[:, 0] > 0
    true = [len(R.runs_of(want[n].numpy())) for n in range(5)]
    cap = max(true[0], true[2], true[4])
    assert min(true[1], true[3]) > cap
    out = tracking.encode_logits_rle(masks, (15, 21), util, max_runs=cap)
    assert calls == [((5, 5, 7), (15, 21), cap)] and byte_calls == [((2, 5, 7), (15, 21), "F")]     # those two, in one call
    assert len(util.packed) == 3 and len(util.seen) == 2
    assert [m["counts"] for m in out] == ["packed1", "rle1", "packed2", "rle2", "packed3"]
    for obj, n in zip(util.packed, (0, 2, 4)):
        assert np.array_equal(R.decode(obj[0]["counts"], 15, 21), want[n].numpy())
    for seen, n in zip(util.seen, (1, 3)):
        assert np.array_equal(seen, want[n].numpy())
    # nothing over the cap: no byte call at all
    byte_calls.clear()
    out = tracking.encode_logits_rle(masks, (15, 21), util)
    assert byte_calls == [] and len(util.packed) == 3 + 5 and calls[-1] == ((5, 5, 7), (15, 21), 8 * 21 + 1)


def test_encode_mask_with_gpu_rle_takes_a_logit_mask_and_still_takes_a_tensor(monkeypatch):
    import devis_amd
    from devis_amd import ops
    calls = []
    monkeypatch.setattr(ops, "mask_run_lengths", fake_run_lengths(calls))
    tm, mm, _ = rle_modules()
    previous = devis_amd.patch_tracker(tm, mm, gpu_rle=True)
    logits = O.blob_logits(1, 1, 5, 7, 4)[0, 0].float()
    rle = tm.encode_mask(devis_amd.LogitMask(logits, (15, 21)))
    assert calls == [((1, 5, 7), (15, 21), 169)] and rle == {"size": [15, 21], "counts": "packed1"}
    assert tm.mask_util.seen == []
    tensor = torch.rand(15, 21)
    assert tm.encode_mask(tensor) == ("their encode", tensor) and len(calls) == 1
    devis_amd.unpatch_tracker(tm, mm, previous)
    assert tm.encode_mask is previous["encode_mask"]


def test_patch_tracker_without_the_keyword_packs_nothing_and_with_it_needs_frpyobjects(monkeypatch):
    import devis_amd
    from devis_amd import ops
    calls, byte_calls = [], []
    monkeypatch.setattr(ops, "mask_run_lengths", fake_run_lengths(calls))
    monkeypatch.setattr(ops, "binarize_masks", fake_binarize(byte_calls))
    tm, mm, tracker = rle_modules(overlap=2)
    theirs = (tm.Tracker.process_masks, tm.encode_mask, mm.HungarianInferenceMatcher.compute_volumetric_iou_cost,
              mm.HungarianInferenceMatcher.compute_frame_average_iou_cost)
    now = lambda: (tm.Tracker.process_masks, tm.encode_mask, mm.HungarianInferenceMatcher.compute_volumetric_iou_cost,      # noqa: E731
                   mm.HungarianInferenceMatcher.compute_frame_average_iou_cost)
    masks = O.blob_logits(6, 1, 5, 7, 3)[:, 0].float()
    previous = devis_amd.patch_tracker(tm, mm)
    tracker.process_masks(0, 0, (15, 21), masks)
    tm.encode_mask(devis_amd.LogitMask(masks[0], (15, 21)))
    assert tm.mask_util.packed == [] and calls == [] and len(tm.mask_util.seen) == 5 and len(byte_calls) == 2
    devis_amd.unpatch_tracker(tm, mm, previous)
    assert now() == theirs
    # a mask_util that cannot pack: refused at patch time, nothing replaced
    tm.mask_util = StandInMaskUtil()
    with pytest.raises(AttributeError, match="frPyObjects"):
        devis_amd.patch_tracker(tm, mm, gpu_rle=True)
    assert now() == theirs
    devis_amd.unpatch_tracker(tm, mm, devis_amd.patch_tracker(tm, mm))          # the default still takes it
    # with it: all four replaced, all four restored
    tm.mask_util = StandInRleUtil()
    previous = devis_amd.patch_tracker(tm, mm, gpu_rle=True)
    assert set(previous) == {"process_masks", "encode_mask", "compute_volumetric_iou_cost", "compute_frame_average_iou_cost"}
    assert tuple(previous[k] for k in ("process_masks", "encode_mask", "compute_volumetric_iou_cost",
                                       "compute_frame_average_iou_cost")) == theirs
    assert all(n is not t for n, t in zip(now(), theirs))
    devis_amd.unpatch_tracker(tm, mm, previous)
    assert now() == theirs
    with pytest.raises(TypeError):
        devis_amd.patch_tracker(tm, mm, True)           # keyword only


def test_documents_describe_the_encoder():
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "mask_run_lengths" in integration and "gpu_rle=True" in integration and "frPyObjects" in integration
    assert "the host still runs `mask_util.encode` on the byte map" not in integration
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^#+ 13\b", design, re.M) and "maskrle" in design
    assert "maskrle.h" in open(os.path.join(ROOT, "README.md")).read()
