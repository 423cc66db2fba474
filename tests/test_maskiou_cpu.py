"""CPU tests of the clip-stitching operators: the oracle against the reference fixtures and against F.interpolate, the C ABI
of include/maskiou.h (exports, version, argument errors, workspace arithmetic -- no compute calls), the host code (shape
checks, errors), the drop-in tracker and matcher methods and their patch functions, the fake-tensor paths, the share of
pixels the binarise comparison leaves out, and the committed resource table.  The kernels themselves are
tests/test_maskiou_gpu.py."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import maskiou_oracle as O
from conftest import ROOT, golden, golden_names

FIXTURES = golden_names("maskiou_")
F64 = torch.float64


def load_fixture(name):
    d = {k: torch.from_numpy(v) for k, v in golden(name).items()}
    d["size"] = tuple(int(v) for v in d["size"])
    return d


def stock_soft_iou(a, b, size, reduce="volume", eps=1e-6):
    """The stock formulation with torch's own operators: interpolate, sigmoid, one matrix product per frame."""
    pa = F.interpolate(a, size=size, mode="bilinear", align_corners=False).sigmoid().flatten(2)
    pb = F.interpolate(b, size=size, mode="bilinear", align_corners=False).sigmoid().flatten(2)
    inter = torch.einsum("ifk,jfk->fij", pa, pb)
    sa, sb = pa.sum(2).t(), pb.sum(2).t()
    if reduce == "frame":
        return (inter / (sa[:, :, None] + sb[:, None, :] - inter).clamp(min=eps)).mean(0)
    inter, sa, sb = inter.sum(0), sa.sum(0), sb.sum(0)
    return inter / (sa[:, None] + sb[None, :] - inter).clamp(min=eps)


# ---- oracle ----------------------------------------------------------------------------------------------------------

def test_fixtures_cover_the_cases():
    assert FIXTURES == ["maskiou_down", "maskiou_up", "maskiou_video"]
    shapes, spread = {}, []
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 32 << 10
        d = load_fixture(name)
        assert d["a"].dtype == F64 and d["b"].dtype == F64 and d["bits_a"].dtype == torch.bool
        assert d["iou_volume"].dtype == F64 and tuple(d["iou_volume"].shape) == (d["a"].shape[0], d["b"].shape[0])
        shapes[name] = (tuple(d["a"].shape[1:]), d["size"])
        iou = d["iou_volume"]
        assert float(iou[0, 0]) > 0.9 and float(iou[1, 1]) < 1e-3          # the identical and the disjoint pair
        assert torch.equal(d["a"][0], d["b"][0])
        spread.append(iou.flatten())
    spread = torch.cat(spread)          # from near 0 to near 1, and in between
    assert float(spread.min()) < 0.01 and float(spread.max()) > 0.9 and int(((spread > 0.05) & (spread < 0.9)).sum()) >= 5
    assert shapes["maskiou_up"] == ((1, 7, 9), (27, 35))
    assert shapes["maskiou_video"] == ((2, 12, 20), (45, 80))
    assert shapes["maskiou_down"] == ((1, 26, 22), (13, 11))


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_equals_the_reference(name):
    d = load_fixture(name)
    for reduce in ("volume", "frame"):
        want = d["iou_" + reduce]
        # (the reference ran F.interpolate in float64, whose taps are float64 too)
        got = O.soft_iou(d["a"], d["b"], d["size"], reduce, arith=F64)
        assert got.dtype == F64 and float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        stock = stock_soft_iou(d["a"], d["b"], d["size"], reduce)
        assert float((stock - want).abs().max()) <= 1e-12 * float(want.abs().max())
    for side in ("a", "b"):
        maps = d[side]
        p = O.probabilities(maps, d["size"], F64)
        stock = F.interpolate(maps, size=d["size"], mode="bilinear", align_corners=False).sigmoid()
        assert float((p - stock).abs().max()) <= 1e-12
        bits, x = O.binarize(maps.flatten(0, 1), d["size"], F64)
        want = d["bits_" + side].flatten(0, 1)
        # (exact ties exist: halving the disjoint pair's map averages +8 and -8 to a logit of 0 along the region's edge)
        clear = (p.flatten(0, 1) - 0.5).abs() > 1e-12
        assert torch.equal(bits[clear], want[clear]) and float(clear.double().mean()) > 0.98
        assert 0.02 < float(want.double().mean()) < 0.98


def test_oracle_terms_are_the_sums_of_the_stock_maps():
    a, b = O.blob_logits(3, 2, 6, 7, 1), O.blob_logits(4, 2, 6, 7, 2)
    inter, sa, sb = O.terms(a, b, (20, 23), F64)
    pa = F.interpolate(a, size=(20, 23), mode="bilinear", align_corners=False).sigmoid()
    pb = F.interpolate(b, size=(20, 23), mode="bilinear", align_corners=False).sigmoid()
    assert tuple(inter.shape) == (2, 3, 4) and tuple(sa.shape) == (2, 3) and tuple(sb.shape) == (2, 4)
    assert float((inter[1, 2, 3] - (pa[2, 1] * pb[3, 1]).sum()).abs()) <= 1e-10
    assert float((sa[1, 2] - pa[2, 1].sum()).abs()) <= 1e-10 and float((sb[0, 3] - pb[3, 0].sum()).abs()) <= 1e-10
    three = O.soft_iou(a[:, 0], b[:, 0], (20, 23), arith=F64)
    assert torch.equal(three, O.soft_iou(a[:, :1], b[:, :1], (20, 23), arith=F64))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("index", range(len(O.BINARIZE_CASES)))
def test_the_binarise_comparison_leaves_out_few_pixels(index, dtype):
    """tests/test_maskiou_gpu.py compares bits outside ``near_zero``; that set stays under the cap for every case it runs."""
    src, size = O.binarize_case(index, dtype)
    arith = F64 if dtype == F64 else torch.float32
    bits, x = O.binarize(src, size, arith)
    out = O.near_zero(x, src)
    assert float(out.double().mean()) <= O.BINARIZE_CAP
    assert 0.05 < float(bits[~out].double().mean()) < 0.95
    stock = F.interpolate(src.double()[:, None], size=size, mode="bilinear", align_corners=False)[:, 0].sigmoid() > 0.5
    assert torch.equal(stock[~out], bits[~out])


# ---- library ---------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_maskiou_h_declares_and_versions_agree():
    from devis_amd import _maskiou, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "maskiou.h")).read()
    declared = set(re.findall(r"\b(maskiou_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_maskiou.EXPORTED_SYMBOLS) and len(declared) == 6
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _maskiou.load()
    assert lib.maskiou_version() == _maskiou.MASKIOU_ABI_VERSION == int(re.search(r"#define MASKIOU_ABI_VERSION (\d+)", header).group(1))
    names = ("BLOCK", "ROWS", "COLS", "SPLIT_TILES", "MAX_SPLITS", "BIN_PIXELS", "BIN_SRC")
    tiles = tuple(int(re.search(r"#define MASKIOU_TILE_%s (\d+)" % n, header).group(1)) for n in names)
    assert tiles == (_maskiou.TILE_BLOCK, _maskiou.TILE_ROWS, _maskiou.TILE_COLS, _maskiou.TILE_SPLIT_TILES,
                     _maskiou.TILE_MAX_SPLITS, _maskiou.TILE_BIN_PIXELS, _maskiou.TILE_BIN_SRC)
    assert all(_maskiou.tile(t) > 0 for t in tiles) and lib.maskiou_tile(9) == -1
    assert _maskiou.tile(_maskiou.TILE_BIN_PIXELS) % 16 == 0 and _maskiou.tile(_maskiou.TILE_BLOCK) % 32 == 0
    assert dict(re.findall(r"MASKIOU_(F32|F64|BF16|F16) = (\d)", header)) == {"F32": "0", "F64": "1", "BF16": "2", "F16": "3"}
    codes = dict(re.findall(r"MASKIOU_(VOLUME|FRAME|ROW_MAJOR|COL_MAJOR) = (\d)", header))
    assert codes == {"VOLUME": str(_maskiou.VOLUME), "FRAME": str(_maskiou.FRAME), "ROW_MAJOR": str(_maskiou.ROW_MAJOR),
                     "COL_MAJOR": str(_maskiou.COL_MAJOR)}
    assert "rule of maskloss.h" in header and "max(scale" not in header         # the tap rule is referred to, not restated
    assert os.path.join(build.include_dir(), "maskiou.h") in build._headers()
    assert any(s.endswith("maskiou.hip") for s in build.sources())
    assert "maskiou.h" in open(os.path.join(ROOT, "setup.py")).read()


def _shape(**kw):
    from devis_amd import _maskiou
    d = dict(Na=5, Nb=6, F=2, h=12, w=20, H=45, W=80)
    d.update(kw)
    return _maskiou.Shape(**d)


def test_maskiou_argument_errors_without_gpu():
    from devis_amd import _maskiou
    lib = _maskiou.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = ctypes.byref(_shape())
    err = lib.maskiou_last_error

    def pair(dtype=0, reduce=0, a=p, b=p, shape=ok, eps=1e-6, ws=p, inter=p, sa=p, sb=p, iou=p):
        return lib.maskiou_pairwise(dtype, reduce, a, b, shape, eps, ws, inter, sa, sb, iou, None)

    def binar(dtype=0, layout=0, src=p, N=3, h=12, w=20, H=45, W=80, out=p):
        return lib.maskiou_binarize(dtype, layout, src, N, h, w, H, W, out, None)

    for call in (pair, binar):
        assert call(dtype=9) == -1 and b"dtype" in err()
        assert call(dtype=-1) == -1 and b"dtype" in err()
    assert pair(reduce=2) == -1 and b"reduce" in err()
    assert pair(reduce=-1) == -1 and b"reduce" in err()
    assert pair(shape=None) == -1 and b"null pointer" in err()
    for bad in (dict(h=0), dict(H=0), dict(h=-3), dict(H=-1), dict(w=0), dict(W=0), dict(Na=-1), dict(Nb=-1), dict(F=0)):
        assert pair(shape=ctypes.byref(_shape(**bad))) == -1 and b"positive" in err(), bad
    assert pair(shape=ctypes.byref(_shape(H=65536, W=65536))) == -1 and b"31 bits" in err()
    assert pair(shape=ctypes.byref(_shape(h=65536, w=65536))) == -1 and b"31 bits" in err()
    assert pair(shape=ctypes.byref(_shape(F=3, h=32768, w=32768))) == -1 and b"F * h * w" in err()
    assert pair(shape=ctypes.byref(_shape(Na=65536, Nb=65536))) == -1 and b"Na * Nb" in err()
    for eps in (-1.0, float("nan"), float("inf")):
        assert pair(eps=eps) == -1 and b"eps" in err(), eps
    for name in ("a", "b", "ws", "inter", "sa", "sb", "iou"):
        assert pair(**{name: None}) == -1 and b"null pointer" in err(), name
    # no map on one side: nothing is launched, nothing is dereferenced
    for empty in (dict(Na=0), dict(Nb=0), dict(Na=0, Nb=0)):
        assert pair(a=None, b=None, ws=None, inter=None, sa=None, sb=None, iou=None, shape=ctypes.byref(_shape(**empty))) == 0
    assert binar(layout=2) == -1 and b"layout" in err()
    assert binar(layout=-1) == -1 and b"layout" in err()
    for bad in (dict(h=0), dict(H=0), dict(w=-2), dict(W=0), dict(N=-1)):
        assert binar(**bad) == -1 and b"positive" in err(), bad
    assert binar(H=65536, W=65536) == -1 and b"31 bits" in err()
    for name in ("src", "out"):
        assert binar(**{name: None}) == -1 and b"null pointer" in err(), name
    assert binar(N=0, src=None, out=None) == 0


def test_workspace_arithmetic():
    from devis_amd import _maskiou
    lib = _maskiou.load()
    th, tw = _maskiou.tile(_maskiou.TILE_ROWS), _maskiou.tile(_maskiou.TILE_COLS)
    least, most = _maskiou.tile(_maskiou.TILE_SPLIT_TILES), _maskiou.tile(_maskiou.TILE_MAX_SPLITS)
    up = lambda n: (n + 255) // 256 * 256      # noqa: E731

    def want(acc, Na, Nb, F_, H, W):
        tiles = -(-H // th) * -(-W // tw)
        per = max(least, -(-tiles // most))
        return up(F_ * -(-tiles // per) * (Na * Nb + Na + Nb) * acc)

    for dtype, acc in ((0, 4), (1, 8), (2, 4), (3, 4)):
        for kw in (dict(), dict(H=th, W=tw), dict(H=th, W=tw * least), dict(H=th, W=tw * least + 1),
                   dict(H=th, W=2 * tw * least + 1), dict(H=th * most, W=tw * least), dict(H=th * most, W=tw * least + 1),
                   dict(Na=100, Nb=100, H=720, W=1280), dict(Na=1, Nb=1, F=1, H=1, W=1)):
            s = _shape(**kw)
            assert lib.maskiou_workspace_bytes(dtype, ctypes.byref(s)) == want(acc, s.Na, s.Nb, s.F, s.H, s.W) > 0, kw
    assert _maskiou.splits(th, tw * least) == (least, least, 1) and _maskiou.splits(th, tw * least + 1) == (least + 1, least, 2)
    assert _maskiou.splits(th, 2 * tw * least + 1)[2] == 3
    assert _maskiou.splits(th * most, tw * least)[1:] == (least, most) and _maskiou.splits(th * most, tw * least + 1)[1] == least + 1
    # the stitching of 100 x 100 tracks at 720 x 1280 stays in the tens of MB
    assert lib.maskiou_workspace_bytes(0, ctypes.byref(_shape(Na=100, Nb=100, H=720, W=1280))) < 32 << 20
    assert lib.maskiou_workspace_bytes(0, ctypes.byref(_shape(Na=0))) == 0 == lib.maskiou_workspace_bytes(0, ctypes.byref(_shape(Nb=0)))
    assert lib.maskiou_workspace_bytes(7, ctypes.byref(_shape())) == -1 and lib.maskiou_workspace_bytes(0, None) == -1
    with pytest.raises(RuntimeError, match="positive"):
        _maskiou.workspace_bytes(0, _shape(w=0))


def test_the_resource_table_shows_no_scratch_in_any_instantiation():
    lines = [ln for ln in open(os.path.join(ROOT, "profiles", "maskiou_resource_usage.txt")) if not ln.startswith("#")]
    kernels = {}
    for ln in lines:
        name, rest = ln.split(":", 1)
        kernels[name] = rest
        assert " 0 VGPR spills, 0 SGPR spills, 0 scratch," in rest, ln
    for kernel, count in (("pairwise_kernel", 4), ("combine_kernel", 2), ("binarize_kernel", 4)):
        assert sum(kernel in k for k in kernels) == count, kernel
    assert len(kernels) == 10


# ---- host ------------------------------------------------------------------------------------------------------------

def test_operators_raise_on_cpu_tensors_and_on_bad_arguments_before_any_launch(monkeypatch):
    import devis_amd
    from devis_amd import _maskiou
    from devis_amd.functions import mask_iou as I

    def no_launch(*a, **k):
        raise AssertionError("a kernel call was made")

    monkeypatch.setattr(_maskiou, "pairwise", no_launch)
    monkeypatch.setattr(_maskiou, "binarize", no_launch)
    a, b = torch.zeros(3, 2, 6, 10), torch.zeros(4, 2, 6, 10)
    for fn in (devis_amd.mask_soft_iou, devis_amd.mask_soft_iou_terms):
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            fn(a, b, (24, 40))
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            fn(a[:, 0], b[:, 0], (24, 40))
        with pytest.raises(RuntimeError, match="b has maps of"):
            fn(a, torch.zeros(4, 3, 6, 10), (24, 40))
        with pytest.raises(RuntimeError, match="b has maps of"):
            fn(a, torch.zeros(4, 2, 6, 11), (24, 40))
        with pytest.raises(RuntimeError, match="a is torch.float32, b is torch.float64"):
            fn(a, b.double(), (24, 40))
        with pytest.raises(RuntimeError, match="must be \\[N, F, h, w\\]"):
            fn(a, b[:, 0], (24, 40))
        with pytest.raises(RuntimeError, match="size must be"):
            fn(a, b, (24, 40, 2))
        with pytest.raises(RuntimeError, match="is empty"):
            fn(a, b, (24, 0))
        with pytest.raises(RuntimeError, match="unsupported dtype"):
            fn(a.long(), b.long(), (24, 40))
        with pytest.raises(RuntimeError, match="mask_soft_iou: a requires a gradient"):
            fn(a.clone().requires_grad_(True), b, (24, 40))
        with pytest.raises(RuntimeError, match="mask_soft_iou: b requires a gradient"):
            fn(a, b.clone().requires_grad_(True), (24, 40))
        with torch.no_grad(), pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            fn(a.clone().requires_grad_(True), b, (24, 40))             # under no_grad the gradient flag is no objection
    with pytest.raises(ValueError, match="reduce"):
        devis_amd.mask_soft_iou(a, b, (24, 40), reduce="mean")
    for eps in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            devis_amd.mask_soft_iou(a, b, (24, 40), eps=eps)
    src = torch.zeros(3, 6, 10)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.binarize_masks(src, (24, 40))
    with pytest.raises(ValueError, match="order"):
        devis_amd.binarize_masks(src, (24, 40), order="K")
    with pytest.raises(RuntimeError, match="src must be \\[N, h, w\\]"):
        devis_amd.binarize_masks(src[0], (24, 40))
    with pytest.raises(RuntimeError, match="binarize_masks: src requires a gradient"):
        devis_amd.binarize_masks(src.clone().requires_grad_(True), (24, 40))
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        devis_amd.binarize_masks(src.to(torch.int32), (24, 40))
    for name in ("mask_soft_iou", "mask_soft_iou_terms", "binarize_masks", "LogitMask", "patch_tracker", "unpatch_tracker"):
        assert name in devis_amd.__all__ and hasattr(devis_amd, name)
    assert devis_amd.mask_soft_iou is devis_amd.ops.mask_soft_iou and devis_amd.binarize_masks is devis_amd.ops.binarize_masks

    meta = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="meta")      # noqa: E731
    assert I.check_pair(meta(3, 2, 6, 10), meta(4, 2, 6, 10), (24, 40)) == (3, 4, 2, 6, 10, 24, 40)
    assert I.check_pair(meta(0, 2, 6, 10, dtype=torch.bfloat16), meta(4, 2, 6, 10, dtype=torch.bfloat16), [5, 5])[:2] == (0, 4)
    assert I.check_src(meta(3, 6, 10, dtype=torch.float16), (24, 40)) == (3, 6, 10, 24, 40)
    bad = [
        ("would be empty", lambda: I.check_pair(meta(3, 2, 0, 10), meta(4, 2, 0, 10), (24, 40))),
        ("would be empty", lambda: I.check_pair(meta(3, 0, 6, 10), meta(4, 0, 6, 10), (24, 40))),
        ("would be empty", lambda: I.check_src(meta(3, 6, 0), (24, 40))),
        ("is empty", lambda: I.check_src(meta(3, 6, 10), (0, 40))),
    ]
    for match, call in bad:
        with pytest.raises(RuntimeError, match=match):
            call()


# ---- the drop-in tracker and matcher methods and their patch -------------------------------------------------------------

class StandInTrack:
    """The accessors of the reference's Track the matcher uses (the suite's own)."""

    def __init__(self, track_id, masks, start_idx=0, last_t=None):
        self._id, self.masks, self.start_idx = track_id, list(masks), start_idx
        self.last_t = len(self.masks) if last_t is None else last_t
        self.mask_id = track_id

    def get_last_results(self, t_window, attr):
        return getattr(self, attr)[self.last_t - t_window: self.last_t]

    def get_first_results(self, t_window, attr):
        return getattr(self, attr)[self.start_idx: self.start_idx + t_window]

    def get_last_t_result(self, t, attr):
        return getattr(self, attr)[self.last_t + t]

    def get_first_t_result(self, t, attr):
        return getattr(self, attr)[self.start_idx + t]

    def get_mask_id(self):
        return self.mask_id


class StandInMaskUtil:
    """Records what it is asked to encode."""

    def __init__(self):
        self.seen = []

    def encode(self, bits):
        self.seen.append(bits)
        return {"size": list(bits.shape), "counts": b"rle%d" % len(self.seen)}


def stand_in_modules(overlap=2, use_binary_mask_iou=False):
    """(tracker module, matcher module, a tracker) of stand-in classes with the reference's names."""
    class HungarianInferenceMatcher:
        def __init__(self):
            self.overlap_w, self.use_binary_mask_iou = overlap, use_binary_mask_iou

        def compute_volumetric_iou_cost(self, track1, track2):
            return "their volume"

        def compute_frame_average_iou_cost(self, track1, track2):
            return "their frame"

    class Tracker:
        def __init__(self, matcher):
            self.hungarian_matcher, self.overlap_window = matcher, overlap

        def process_masks(self, start_idx, idx, tgt_size, masks):
            return "theirs"

    def encode_mask(mask):
        return ("their encode", mask)

    tracker_module = types.SimpleNamespace(Tracker=Tracker, encode_mask=encode_mask, mask_util=StandInMaskUtil())
    matcher_module = types.SimpleNamespace(HungarianInferenceMatcher=HungarianInferenceMatcher)
    return tracker_module, matcher_module, Tracker(HungarianInferenceMatcher())


def reference_choice(use_binary_mask_iou, overlap_window, start_idx, idx, num_masks):
    """The reference's branches of process_masks, written out: True where a frame is encoded at once."""
    out = []
    for t in range(num_masks):
        if use_binary_mask_iou:
            out.append(True)
        elif idx == 0:
            out.append(t < num_masks - overlap_window)
        else:
            out.append(overlap_window + start_idx <= t < num_masks - overlap_window or t < start_idx)
    return out


def fake_binarize(calls):
    def binarize_masks(src, size, *, order="C"):
        calls.append((tuple(src.shape), tuple(size), order))
        bits = F.interpolate(src[:, None].float(), size=tuple(size), mode="bilinear", align_corners=False)[:, 0] > 0
        return bits.transpose(1, 2).contiguous().transpose(1, 2) if order == "F" else bits
    return binarize_masks


@pytest.mark.parametrize("binary", [False, True])
def test_process_masks_encodes_and_keeps_the_frames_the_reference_does(binary, monkeypatch):
    import devis_amd
    from devis_amd import ops
    calls = []
    monkeypatch.setattr(ops, "binarize_masks", fake_binarize(calls))
    tm, mm, tracker = stand_in_modules(overlap=2, use_binary_mask_iou=binary)
    previous = devis_amd.patch_tracker(tm, mm)
    masks = O.blob_logits(6, 1, 5, 7, 3)[:, 0].float()
    for start_idx, idx in ((0, 0), (0, 1), (1, 2), (3, 1)):
        calls.clear()
        tm.mask_util.seen.clear()
        out = tracker.process_masks(start_idx, idx, (15, 21), masks)
        choice = reference_choice(binary, 2, start_idx, idx, 6)
        assert [isinstance(m, dict) for m in out] == choice
        assert [isinstance(m, devis_amd.LogitMask) for m in out] == [not c for c in choice]
        assert calls == ([((sum(choice), 5, 7), (15, 21), "F")] if any(choice) else [])      # one binarise call
        assert len(tm.mask_util.seen) == sum(choice)
        want = F.interpolate(masks[:, None], size=(15, 21), mode="bilinear", align_corners=False)[:, 0] > 0
        k = 0
        for t, m in enumerate(out):
            if choice[t]:
                seen = tm.mask_util.seen[k]
                k += 1
                assert seen.shape == (15, 21) and seen.flags["F_CONTIGUOUS"] and seen.dtype == np.bool_
                assert np.array_equal(seen, want[t].numpy()) and m["counts"] == "rle%d" % k and isinstance(m["counts"], str)
            else:
                assert torch.equal(m.logits, masks[t]) and m.size == (15, 21) and not isinstance(m, dict) and m is not None
                stock = F.interpolate(masks[t][None, None], (15, 21), mode="bilinear", align_corners=False).sigmoid()[0, 0]
                assert torch.equal(m.probabilities(), stock)
    devis_amd.unpatch_tracker(tm, mm, previous)
    assert tracker.process_masks(0, 0, (15, 21), masks) == "theirs"


def test_encode_mask_takes_a_logit_mask_and_still_takes_a_tensor(monkeypatch):
    import devis_amd
    from devis_amd import ops
    calls = []
    monkeypatch.setattr(ops, "binarize_masks", fake_binarize(calls))
    tm, mm, _ = stand_in_modules()
    previous = devis_amd.patch_tracker(tm, mm)
    logits = O.blob_logits(1, 1, 5, 7, 4)[0, 0].float()
    rle = tm.encode_mask(devis_amd.LogitMask(logits, (15, 21)))
    assert calls == [((1, 5, 7), (15, 21), "F")] and rle["counts"] == "rle1" and rle["size"] == [15, 21]
    tensor = torch.rand(15, 21)
    assert tm.encode_mask(tensor) == ("their encode", tensor) and len(calls) == 1
    with pytest.raises(ValueError, match="\\[h, w\\]"):
        devis_amd.LogitMask(torch.zeros(1, 5, 7), (15, 21))
    devis_amd.unpatch_tracker(tm, mm, previous)
    assert tm.encode_mask is previous["encode_mask"]


@pytest.mark.parametrize("reduce", ["volume", "frame"])
def test_iou_cost_is_one_operator_call_on_the_stacked_logits(reduce, monkeypatch):
    import devis_amd
    from devis_amd import ops
    calls = []

    def fake(a, b, size, *, reduce="volume", eps=1e-6):
        calls.append((a, b, tuple(size), reduce, eps))
        return stock_soft_iou(a, b, tuple(size), reduce, eps)

    monkeypatch.setattr(ops, "mask_soft_iou", fake)
    tm, mm, tracker = stand_in_modules(overlap=2)
    previous = devis_amd.patch_tracker(tm, mm)
    matcher = tracker.hungarian_matcher
    a, b = O.blob_logits(3, 4, 5, 7, 5).float(), O.blob_logits(4, 3, 5, 7, 6).float()
    wrap = lambda maps: [devis_amd.LogitMask(m, (15, 21)) for m in maps]      # noqa: E731
    video = [StandInTrack(i, [None] + wrap(a[i]), last_t=4) for i in range(3)]       # the last two frames before last_t = 4
    clip = [StandInTrack(j, wrap(b[j]), start_idx=1) for j in range(4)]              # the two frames from start_idx = 1
    fn = matcher.compute_volumetric_iou_cost if reduce == "volume" else matcher.compute_frame_average_iou_cost
    cost = fn(video, clip)
    assert len(calls) == 1 and calls[0][2:] == ((15, 21), reduce, 1e-6)
    assert torch.equal(calls[0][0], a[:, 1:3]) and torch.equal(calls[0][1], b[:, 1:3])
    assert isinstance(cost, np.ndarray) and cost.dtype == np.float64 and cost.shape == (3, 4)
    assert np.allclose(cost, stock_soft_iou(a[:, 1:3], b[:, 1:3], (15, 21), reduce).numpy(), atol=1e-6)
    assert fn([], clip).shape == (0, 4) and fn(video, []).shape == (3, 0) and len(calls) == 1
    video[1].masks[3] = None
    with pytest.raises(TypeError):
        fn(video, clip)
    video[1].masks[3] = devis_amd.LogitMask(a[1, 2], (15, 22))
    with pytest.raises(RuntimeError, match="different sizes"):
        fn(video, clip)
    matcher.use_binary_mask_iou = True
    assert fn(video, clip) == "their " + reduce and len(calls) == 1          # the fall-through
    devis_amd.unpatch_tracker(tm, mm, previous)
    assert mm.HungarianInferenceMatcher.compute_volumetric_iou_cost is previous["compute_volumetric_iou_cost"]


def test_patch_tracker_sets_and_restores_and_leaves_the_other_patches_alone():
    import devis_amd

    class TheirHead(torch.nn.Module):
        pass

    tm, mm, tracker = stand_in_modules()
    crit = types.SimpleNamespace(SetCriterion=type("SetCriterion", (), {"loss_masks": lambda self: "theirs"}))
    seg = types.SimpleNamespace(MaskHeadConv=TheirHead, ModulatedDeformableConv2d=TheirHead, MultiScaleMHAttentionMap=TheirHead)
    theirs = (tm.Tracker.process_masks, tm.encode_mask, mm.HungarianInferenceMatcher.compute_volumetric_iou_cost,
              mm.HungarianInferenceMatcher.compute_frame_average_iou_cost)
    loss = crit.SetCriterion.loss_masks
    previous = devis_amd.patch_tracker(tm, mm)
    assert set(previous) == {"process_masks", "encode_mask", "compute_volumetric_iou_cost", "compute_frame_average_iou_cost"}
    assert tuple(previous[k] for k in ("process_masks", "encode_mask", "compute_volumetric_iou_cost",
                                       "compute_frame_average_iou_cost")) == theirs
    now = (tm.Tracker.process_masks, tm.encode_mask, mm.HungarianInferenceMatcher.compute_volumetric_iou_cost,
           mm.HungarianInferenceMatcher.compute_frame_average_iou_cost)
    assert all(n is not t for n, t in zip(now, theirs))
    assert tracker.process_masks.__func__ is tm.Tracker.process_masks           # trackers that exist follow
    assert (seg.MaskHeadConv, seg.ModulatedDeformableConv2d, seg.MultiScaleMHAttentionMap) == (TheirHead,) * 3
    assert crit.SetCriterion.loss_masks is loss
    undo = devis_amd.patch_mask_losses(crit)           # another patch does not touch the tracker
    assert tm.Tracker.process_masks is now[0] and tm.encode_mask is now[1]
    devis_amd.unpatch_mask_losses(crit, undo)
    devis_amd.unpatch_tracker(tm, mm, previous)
    assert (tm.Tracker.process_masks, tm.encode_mask, mm.HungarianInferenceMatcher.compute_volumetric_iou_cost,
            mm.HungarianInferenceMatcher.compute_frame_average_iou_cost) == theirs
    assert tracker.hungarian_matcher.compute_volumetric_iou_cost(None, None) == "their volume"
    with pytest.raises(AttributeError):
        devis_amd.patch_tracker(types.SimpleNamespace(), mm)


# ---- fake-tensor paths -----------------------------------------------------------------------------------------------

def _nodes(graph, name):
    return [n for n in graph.nodes if n.op == "call_function" and name in str(n.target)]


def test_make_fx_with_fake_tensors_gives_one_op_node():
    from torch.fx.experimental.proxy_tensor import make_fx
    from devis_amd import ops
    meta = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")      # noqa: E731
    for dtype, acc in ((torch.float32, torch.float32), (torch.bfloat16, torch.float32), (torch.float64, torch.float64)):
        gm = make_fx(lambda a, b: ops.mask_soft_iou_op(a, b, [45, 80], "frame", 1e-6), tracing_mode="fake")(
            meta(5, 2, 12, 20, dtype=dtype), meta(7, 2, 12, 20, dtype=dtype))
        nodes = _nodes(gm.graph, "mask_soft_iou")
        assert len(nodes) == 1
        iou, inter, sa, sb = nodes[0].meta["val"]
        assert tuple(iou.shape) == (5, 7) and tuple(inter.shape) == (2, 5, 7) and tuple(sa.shape) == (2, 5) and tuple(sb.shape) == (2, 7)
        assert iou.dtype == inter.dtype == sa.dtype == sb.dtype == acc
        for order, strides in (("C", (45 * 80, 80, 1)), ("F", (45 * 80, 1, 45))):
            gm = make_fx(lambda s: ops.binarize_masks_op(s, [45, 80], order), tracing_mode="fake")(meta(5, 12, 20, dtype=dtype))      # noqa: B023
            nodes = _nodes(gm.graph, "binarize_masks")
            assert len(nodes) == 1
            val = nodes[0].meta["val"]
            assert tuple(val.shape) == (5, 45, 80) and val.dtype == torch.bool and val.stride() == strides
    with pytest.raises(Exception, match="reduce"):
        make_fx(lambda a, b: ops.mask_soft_iou_op(a, b, [45, 80], "mean", 1e-6), tracing_mode="fake")(meta(5, 2, 12, 20), meta(7, 2, 12, 20))


@pytest.mark.parametrize("dynamic", [False, True])
def test_export_gives_one_op_node_for_static_and_dynamic_sizes(dynamic):
    import devis_amd

    class Pair(torch.nn.Module):
        def forward(self, a, b):
            return devis_amd.mask_soft_iou(a, b, (45, 80), reduce="frame")

    class Bits(torch.nn.Module):
        def forward(self, src):
            return devis_amd.binarize_masks(src, (45, 80), order="F")

    D = torch.export.Dim
    args = (torch.empty(5, 2, 12, 20, device="meta"), torch.empty(7, 2, 12, 20, device="meta"))
    shapes = None
    if dynamic:
        Na, Nb, Fr, h, w = D("Na", min=2, max=512), D("Nb", min=2, max=512), D("Fr", min=2, max=16), D("h", min=2, max=512), D("w", min=2, max=512)
        shapes = ({0: Na, 1: Fr, 2: h, 3: w}, {0: Nb, 1: Fr, 2: h, 3: w})
    ep = torch.export.export(Pair(), args, dynamic_shapes=shapes)
    nodes = _nodes(ep.graph, "mask_soft_iou")
    assert len(nodes) == 1
    iou = nodes[0].meta["val"][0]
    assert len(iou.shape) == 2
    if dynamic:
        assert not isinstance(iou.shape[0], int) and not isinstance(iou.shape[1], int)
    else:
        assert tuple(iou.shape) == (5, 7)
    shapes = ({0: D("N", min=2, max=512), 1: D("h", min=2, max=512), 2: D("w", min=2, max=512)},) if dynamic else None
    ep = torch.export.export(Bits(), (torch.empty(5, 12, 20, device="meta"),), dynamic_shapes=shapes)
    nodes = _nodes(ep.graph, "binarize_masks")
    assert len(nodes) == 1
    val = nodes[0].meta["val"]
    assert tuple(val.shape)[1:] == (45, 80) and val.dtype == torch.bool
    assert isinstance(val.shape[0], int) != dynamic
