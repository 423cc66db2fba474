"""CPU tests of the binary mask IoU: the numpy oracle on hand-written cases, the C ABI of include/maskbiou.h (exports,
version, argument errors, workspace arithmetic -- no compute calls), the one definition of the bits pass, the host code (shape
checks, errors, fake tensors, export), the tracker wiring with ``gpu_binary_iou=True`` on a fake operator, the committed
resource table and the documents.  The kernels themselves are tests/test_maskbiou_gpu.py."""
import ctypes
import glob
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import maskbiou_oracle as B
import maskiou_oracle as O
from conftest import ROOT
from test_maskiou_cpu import StandInMaskUtil, StandInTrack, fake_binarize, reference_choice, stand_in_modules


# ---- oracle ----------------------------------------------------------------------------------------------------------

def _box(y0, y1, x0, x1, shape=(6, 8)):
    m = np.zeros(shape, bool)
    m[y0:y1, x0:x1] = True
    return m


def test_oracle_on_hand_written_cases():
    left, right, big, small, none = _box(0, 6, 0, 3), _box(0, 6, 5, 8), _box(1, 5, 1, 7), _box(2, 4, 2, 5), _box(0, 0, 0, 0)
    A = np.stack([left, big, none, left])[:, None]              # [4, 1, 6, 8]
    Bm = np.stack([right, left, small, none])[:, None]
    inter, area_a, area_b = B.counts_of_bits(A, Bm)
    assert inter.shape == (4, 4, 1) and area_a.shape == (4, 1) and area_b.shape == (4, 1)
    assert area_a[:, 0].tolist() == [18, 24, 0, 18] and area_b[:, 0].tolist() == [18, 18, 6, 0]
    assert inter[0, 0, 0] == 0 and inter[0, 1, 0] == 18 and inter[1, 2, 0] == 6 and inter[1, 1, 0] == 8
    for reduce in ("volume", "frame"):
        iou = B.iou(inter, area_a, area_b, reduce)
        assert iou.dtype == np.float64 and iou.shape == (4, 4)
        assert iou[0, 0] == 0.0                                 # disjoint
        assert iou[0, 1] == 1.0                                 # equal
        assert iou[1, 2] == 6 / 24                              # nested: the inner area over the outer
        assert iou[1, 1] == 8 / (24 + 18 - 8)
        assert iou[2, 3] == 0.0                                 # both empty: 0.0, not a division by 0
        assert iou[2, 0] == 0.0 and iou[0, 3] == 0.0            # one empty
    # two frames: "volume" divides the sums, "frame" averages the ratios
    A2, B2 = np.stack([left, big])[None], np.stack([left, small])[None]          # [1, 2, 6, 8]
    terms = B.counts_of_bits(A2, B2)
    assert B.iou(*terms, "volume")[0, 0] == (18 + 6) / (18 + 24) and B.iou(*terms, "frame")[0, 0] == (1.0 + 0.25) / 2
    # the reference's pair function: truthiness branches and a frame without a detection
    assert B.reference_iou([left, big], [left, small]) == (18 + 6) / (18 + 24)
    assert B.reference_iou([left, None], [left, small]) == 18 / (18 + 6)        # None adds the other mask's area to the union
    assert B.reference_iou([left, big], [None, small]) == 6 / (18 + 24)
    assert B.reference_iou([None, None], [None, None]) == 0.0 and B.reference_iou([none], [none]) == 0.0
    assert B.reference_iou([None], [left]) == 0.0
    # a None frame is an empty mask: the same numbers from the counts
    for d, g in (([left, None], [left, small]), ([left, big], [None, small]), ([None, None], [left, None])):
        as_bits = lambda w: np.stack([none if m is None else m for m in w])[None]      # noqa: E731
        terms = B.counts_of_bits(as_bits(d), as_bits(g))
        assert B.iou(*terms, "volume")[0, 0] == B.reference_iou(d, g)
        assert B.reference_volume([d], [g])[0, 0] == B.reference_iou(d, g)
        assert B.iou(*terms, "frame")[0, 0] == B.reference_frame([d], [g])[0, 0]


def test_oracle_counts_are_those_of_the_stock_upsample():
    a, b = O.blob_logits(3, 2, 6, 7, 1).float(), O.blob_logits(4, 2, 6, 7, 2).float()
    inter, area_a, area_b = B.counts(a, b, (20, 23))
    pa = F.interpolate(a, size=(20, 23), mode="bilinear", align_corners=False) > 0
    pb = F.interpolate(b, size=(20, 23), mode="bilinear", align_corners=False) > 0
    assert inter.shape == (3, 4, 2) and inter[2, 3, 1] == int((pa[2, 1] & pb[3, 1]).sum())
    assert area_a[2, 1] == int(pa[2, 1].sum()) and area_b[3, 0] == int(pb[3, 0].sum())
    iou = B.iou(inter, area_a, area_b, "volume")
    assert 0.0 <= iou.min() and iou.max() <= 1.0 and iou.max() > 0.0


# ---- library ---------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_maskbiou_h_declares_and_versions_agree():
    from devis_amd import _maskbiou, _maskiou, _maskrle, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "maskbiou.h")).read()
    declared = set(re.findall(r"\b(maskbiou_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_maskbiou.EXPORTED_SYMBOLS) and len(declared) == 5
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _maskbiou.load()
    assert lib.maskbiou_version() == _maskbiou.MASKBIOU_ABI_VERSION == int(re.search(r"#define MASKBIOU_ABI_VERSION (\d+)", header).group(1))
    names = ("BLOCK", "CHUNK_WORDS", "SPLIT_WORDS")
    tiles = tuple(int(re.search(r"#define MASKBIOU_TILE_%s (\d+)" % n, header).group(1)) for n in names)
    assert tiles == (_maskbiou.TILE_BLOCK, _maskbiou.TILE_CHUNK_WORDS, _maskbiou.TILE_SPLIT_WORDS)
    assert all(_maskbiou.tile(t) > 0 for t in tiles) and lib.maskbiou_tile(9) == -1
    assert _maskbiou.tile(_maskbiou.TILE_SPLIT_WORDS) % _maskbiou.tile(_maskbiou.TILE_CHUNK_WORDS) == 0
    assert dict(re.findall(r"MASKBIOU_(F32|F64|BF16|F16) = (\d)", header)) == {"F32": "0", "F64": "1", "BF16": "2", "F16": "3"}
    for phrase in ("inter  [Na, Nb, F]", "area_a [Na, F]", "area_b [Nb, F]", "maskiou_binarize", "rule of maskloss.h", "atomic"):
        assert phrase in header, phrase
    assert "max(scale" not in header and "0.5" not in header              # the tap rule is referred to, not restated
    assert os.path.join(build.include_dir(), "maskbiou.h") in build._headers()
    assert any(s.endswith("maskbiou.hip") for s in build.sources())
    assert "maskbiou.h" in open(os.path.join(ROOT, "setup.py")).read() and "maskbiou.h" in build.include_dir.__doc__
    # the siblings are as they were
    rle = open(os.path.join(ROOT, "include", "maskrle.h")).read()
    assert len(set(re.findall(r"\b(maskrle_[a-z_0-9]+)\s*\(", rle))) == 5 == len(_maskrle.EXPORTED_SYMBOLS)
    assert "#define MASKRLE_ABI_VERSION 1\n" in rle and _maskrle.load().maskrle_version() == 1
    iou = open(os.path.join(ROOT, "include", "maskiou.h")).read()
    assert len(set(re.findall(r"\b(maskiou_[a-z_0-9]+)\s*\(", iou))) == 6 == len(_maskiou.EXPORTED_SYMBOLS)
    assert "#define MASKIOU_ABI_VERSION 1\n" in iou and _maskiou.load().maskiou_version() == 1


def test_the_bits_pass_has_one_definition():
    csrc = os.path.join(ROOT, "devis_amd", "csrc")
    defining, launching = [], []
    for path in sorted(glob.glob(os.path.join(csrc, "*"))):
        text = open(path).read()
        if re.search(r"\bvoid\s+bits_kernel\s*\(", text):
            defining.append(os.path.basename(path))
        if "bits_kernel<" in text:
            launching.append(os.path.basename(path))
        if os.path.basename(path) != "mask_bits.h":
            assert not re.search(r"\bint\s+words_of\s*\(", text) and "kBitsTile =" not in text, path
    assert defining == ["mask_bits.h"] and launching == ["maskbiou.hip", "maskrle.hip"]
    for name in ("maskbiou.hip", "maskrle.hip"):
        assert '#include "mask_bits.h"' in open(os.path.join(csrc, name)).read()
    bits = open(os.path.join(csrc, "mask_bits.h")).read()
    assert '#include "mask_taps.h"' in bits and "Tap<A> tap_at(" not in bits and " A lerp_of(" not in bits


def test_maskbiou_argument_errors_without_gpu():
    from devis_amd import _maskbiou
    lib = _maskbiou.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.maskbiou_last_error

    def counts(dtype=0, a=p, b=p, Na=3, Nb=4, F=2, h=12, w=20, H=45, W=80, ws=p, inter=p, area_a=p, area_b=p):
        return lib.maskbiou_counts(dtype, a, b, Na, Nb, F, h, w, H, W, ws, inter, area_a, area_b, None)

    for dtype in (9, -1, 4):
        assert counts(dtype=dtype) == -1 and b"dtype" in err()
    for bad in (dict(h=0), dict(H=0), dict(w=-2), dict(W=0), dict(h=-1), dict(H=-7), dict(Na=-1), dict(Nb=-1), dict(F=0), dict(F=-1)):
        assert counts(**bad) == -1 and b"positive" in err(), bad
    assert counts(H=65536, W=65536) == -1 and b"31 bits" in err()
    assert counts(H=32768, W=65536) == -1 and b"31 bits" in err()           # 2^31 itself
    assert counts(h=65536, w=65536) == -1 and b"31 bits" in err()
    assert counts(Na=65536, Nb=65536) == -1 and b"Na * Nb * F" in err()
    assert counts(Na=32768, Nb=32768, F=2) == -1 and b"Na * Nb * F" in err()
    assert counts(Na=2 ** 30, Nb=1, F=2) == -1 and b"31 bits" in err()
    for name in ("a", "b", "ws", "inter", "area_a", "area_b"):
        assert counts(**{name: None}) == -1 and b"null pointer" in err(), name
    # no map on one side: nothing is launched, nothing is dereferenced
    for empty in (dict(Na=0), dict(Nb=0), dict(Na=0, Nb=0)):
        assert counts(a=None, b=None, ws=None, inter=None, area_a=None, area_b=None, **empty) == 0 and err() == b""
    assert counts(Na=0, F=0) == -1                                            # (checked before the no-op)


def test_workspace_arithmetic():
    from devis_amd import _maskbiou
    lib = _maskbiou.load()
    up = lambda n: (n + 255) // 256 * 256      # noqa: E731
    for Na, Nb, F_, H, W in ((1, 1, 1, 1, 1), (1, 2, 1, 8, 8), (3, 4, 2, 5, 13), (7, 2, 3, 67, 61), (100, 100, 2, 720, 1280),
                             (1, 1, 1, 32767, 65536), (1, 1, 2, 1, 2 ** 31 - 1)):
        got = lib.maskbiou_workspace_bytes(Na, Nb, F_, H, W)
        assert got == up((Na + Nb) * F_ * -(-H * W // 64) * 8) and got % 256 == 0 and got > 0, (Na, Nb, F_, H, W)
    assert lib.maskbiou_workspace_bytes(0, 5, 2, 720, 1280) == 0 == lib.maskbiou_workspace_bytes(5, 0, 2, 720, 1280)
    # one bit per pixel: an eighth of the byte maps
    assert lib.maskbiou_workspace_bytes(100, 100, 2, 720, 1280) <= 400 * 720 * 1280 // 8 + 256
    for bad in ((-1, 4, 1, 4, 4), (4, -1, 1, 4, 4), (1, 1, 0, 4, 4), (1, 1, 1, 0, 4), (1, 1, 1, 4, 0), (1, 1, 1, 65536, 65536),
                (1, 1, 1, 32768, 65536), (65536, 65536, 1, 4, 4), (2 ** 30, 2 ** 30, 1, 4, 4)):
        assert lib.maskbiou_workspace_bytes(*bad) == -1, bad
    with pytest.raises(RuntimeError, match="31 bits"):
        _maskbiou.workspace_bytes(1, 1, 1, 65536, 65536)


def test_the_resource_table_shows_no_scratch_in_any_instantiation():
    lines = [ln for ln in open(os.path.join(ROOT, "profiles", "maskbiou_resource_usage.txt")) if not ln.startswith("#")]
    kernels = {}
    for ln in lines:
        name, rest = ln.split(":", 1)
        kernels[name] = rest
        assert " 0 VGPR spills, 0 SGPR spills, 0 scratch," in rest, ln
    for kernel, count in (("bits_kernel", 4), ("pairs_kernel", 1), ("zero_kernel", 1)):
        assert sum(kernel in k for k in kernels) == count, kernel
    assert len(kernels) == 6
    # the bits pass is the same code in both units: the same names and the same registers
    rle = [ln for ln in open(os.path.join(ROOT, "profiles", "maskrle_resource_usage.txt")) if "bits_kernel" in ln]
    assert sorted(rle) == sorted(ln for ln in lines if "bits_kernel" in ln)


# ---- host ------------------------------------------------------------------------------------------------------------

def test_operators_raise_on_cpu_tensors_and_on_bad_arguments_before_any_launch(monkeypatch):
    import devis_amd
    from devis_amd import _maskbiou
    from devis_amd.functions import mask_binary_iou as M

    def no_launch(*a, **k):
        raise AssertionError("a kernel call was made")

    monkeypatch.setattr(_maskbiou, "counts", no_launch)
    a, b = torch.zeros(3, 2, 6, 10), torch.zeros(4, 2, 6, 10)
    for fn in (devis_amd.mask_binary_iou, devis_amd.mask_binary_iou_terms):
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            fn(a, b, (24, 40))
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            fn(a[:0], b, (24, 40))
        with pytest.raises(RuntimeError, match="b has maps of"):
            fn(a, torch.zeros(4, 3, 6, 10), (24, 40))
        with pytest.raises(RuntimeError, match="b has maps of"):
            fn(a, torch.zeros(4, 2, 6, 11), (24, 40))
        with pytest.raises(RuntimeError, match="a is torch.float32, b is torch.float64"):
            fn(a, b.double(), (24, 40))
        with pytest.raises(RuntimeError, match="must be \\[N, F, h, w\\]"):
            fn(a, b[:, 0], (24, 40))
        with pytest.raises(RuntimeError, match="must be \\[N, F, h, w\\]"):
            fn(a[:, 0], b[:, 0], (24, 40))
        with pytest.raises(RuntimeError, match="size must be"):
            fn(a, b, (24, 40, 2))
        with pytest.raises(RuntimeError, match="is empty"):
            fn(a, b, (24, 0))
        with pytest.raises(RuntimeError, match="31 bits"):
            fn(a, b, (65536, 65536))
        with pytest.raises(RuntimeError, match="unsupported dtype"):
            fn(a.long(), b.long(), (24, 40))
        with pytest.raises(RuntimeError, match="mask_binary_iou: a requires a gradient"):
            fn(a.clone().requires_grad_(True), b, (24, 40))
        with pytest.raises(RuntimeError, match="mask_binary_iou: b requires a gradient"):
            fn(a, b.clone().requires_grad_(True), (24, 40))
        with torch.no_grad(), pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            fn(a.clone().requires_grad_(True), b, (24, 40))             # under no_grad the gradient flag is no objection
    for bad in ("mean", "", None):
        with pytest.raises(ValueError, match="reduce"):
            devis_amd.mask_binary_iou(a, b, (24, 40), reduce=bad)
    with pytest.raises(TypeError):
        devis_amd.mask_binary_iou(a, b, (24, 40), "frame")               # keyword only
    for name in ("mask_binary_iou", "mask_binary_iou_terms"):
        assert name in devis_amd.__all__ and getattr(devis_amd, name) is getattr(devis_amd.ops, name)

    meta = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="meta")      # noqa: E731
    assert M.check_pair(meta(3, 2, 6, 10), meta(4, 2, 6, 10), (24, 40)) == (3, 4, 2, 6, 10, 24, 40)
    assert M.check_pair(meta(0, 2, 6, 10, dtype=torch.bfloat16), meta(4, 2, 6, 10, dtype=torch.bfloat16), [5, 5])[:2] == (0, 4)
    for call in (lambda: M.check_pair(meta(3, 2, 0, 10), meta(4, 2, 0, 10), (24, 40)),
                 lambda: M.check_pair(meta(3, 0, 6, 10), meta(4, 0, 6, 10), (24, 40))):
        with pytest.raises(RuntimeError, match="would be empty"):
            call()
    # the ratio of the host code is the oracle's, on the CPU too (it is plain torch on the counts)
    g = np.random.default_rng(3)
    area_a, area_b = g.integers(0, 50, (3, 2)), g.integers(0, 50, (4, 2))
    inter = np.minimum(g.integers(0, 50, (3, 4, 2)), np.minimum(area_a[:, None], area_b[None]))
    area_a[1], inter[1] = 0, 0
    area_b[2], inter[:, 2] = 0, 0
    for reduce in ("volume", "frame"):
        got = M.ratio(torch.from_numpy(inter).int(), torch.from_numpy(area_a).int(), torch.from_numpy(area_b).int(), reduce)
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), B.iou(inter, area_a, area_b, reduce))
    big = torch.full((1, 1, 3), 2 ** 31 - 1, dtype=torch.int32)         # the sums over the frames are formed in int64
    assert float(M.ratio(big, big[0], big[0], "volume")) == 1.0


def _nodes(graph, name):
    return [n for n in graph.nodes if n.op == "call_function" and name in str(n.target)]


def test_fake_tensors_give_the_shapes_and_dtypes():
    from torch.fx.experimental.proxy_tensor import make_fx
    from devis_amd import ops
    meta = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")      # noqa: E731
    for dtype in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
        args = (meta(5, 2, 12, 20, dtype=dtype), meta(7, 2, 12, 20, dtype=dtype))
        gm = make_fx(lambda a, b: ops.mask_binary_iou_terms_op(a, b, [45, 80]), tracing_mode="fake")(*args)
        nodes = _nodes(gm.graph, "mask_binary_iou_terms")
        assert len(nodes) == 1
        inter, area_a, area_b = nodes[0].meta["val"]
        assert tuple(inter.shape) == (5, 7, 2) and tuple(area_a.shape) == (5, 2) and tuple(area_b.shape) == (7, 2)
        assert inter.dtype == area_a.dtype == area_b.dtype == torch.int32 and inter.is_contiguous()
        for reduce in ("volume", "frame"):
            gm = make_fx(lambda a, b: ops.mask_binary_iou_op(a, b, [45, 80], reduce), tracing_mode="fake")(*args)      # noqa: B023
            nodes = [n for n in _nodes(gm.graph, "mask_binary_iou") if "terms" not in str(n.target)]
            assert len(nodes) == 1
            val = nodes[0].meta["val"]
            assert tuple(val.shape) == (5, 7) and val.dtype == torch.float64 and val.is_contiguous()
    gm = make_fx(lambda a, b: ops.mask_binary_iou_terms_op(a, b, [45, 80]), tracing_mode="fake")(meta(0, 2, 12, 20), meta(7, 2, 12, 20))
    assert [tuple(v.shape) for v in _nodes(gm.graph, "mask_binary_iou_terms")[0].meta["val"]] == [(0, 7, 2), (0, 2), (7, 2)]
    with pytest.raises(Exception, match="reduce"):
        make_fx(lambda a, b: ops.mask_binary_iou_op(a, b, [45, 80], "mean"), tracing_mode="fake")(meta(5, 2, 12, 20), meta(7, 2, 12, 20))
    with pytest.raises(Exception, match="b has maps of"):
        make_fx(lambda a, b: ops.mask_binary_iou_terms_op(a, b, [45, 80]), tracing_mode="fake")(meta(5, 2, 12, 20), meta(7, 3, 12, 20))


@pytest.mark.parametrize("dynamic", [False, True])
def test_export_gives_one_op_node_for_static_and_dynamic_sizes(dynamic):
    import devis_amd

    class Ratio(torch.nn.Module):
        def forward(self, a, b):
            return devis_amd.mask_binary_iou(a, b, (45, 80), reduce="frame")

    class Terms(torch.nn.Module):
        def forward(self, a, b):
            return devis_amd.mask_binary_iou_terms(a, b, (45, 80))

    D = torch.export.Dim
    args = (torch.empty(5, 2, 12, 20, device="meta"), torch.empty(7, 2, 12, 20, device="meta"))
    shapes = None
    if dynamic:
        Na, Nb, Fr, h, w = D("Na", min=2, max=512), D("Nb", min=2, max=512), D("Fr", min=2, max=16), D("h", min=2, max=512), D("w", min=2, max=512)
        shapes = ({0: Na, 1: Fr, 2: h, 3: w}, {0: Nb, 1: Fr, 2: h, 3: w})
    ep = torch.export.export(Ratio(), args, dynamic_shapes=shapes)
    nodes = _nodes(ep.graph, "mask_binary_iou")
    assert len(nodes) == 1 and "terms" not in str(nodes[0].target)
    iou = nodes[0].meta["val"]
    assert len(iou.shape) == 2 and iou.dtype == torch.float64
    assert all(isinstance(s, int) != dynamic for s in iou.shape)
    ep = torch.export.export(Terms(), args, dynamic_shapes=shapes)
    nodes = _nodes(ep.graph, "mask_binary_iou_terms")
    assert len(nodes) == 1
    inter, area_a, area_b = nodes[0].meta["val"]
    assert len(inter.shape) == 3 and len(area_a.shape) == 2 and inter.dtype == area_b.dtype == torch.int32
    if not dynamic:
        assert tuple(inter.shape) == (5, 7, 2) and tuple(area_a.shape) == (5, 2) and tuple(area_b.shape) == (7, 2)


# ---- the tracker wiring with gpu_binary_iou=True -------------------------------------------------------------------------

def binary_modules(overlap=2, use_binary_mask_iou=True):
    """The stand-in modules with a ``Track`` that has the reference's ``encode_all_masks`` and ``get_formatted_result``."""
    tm, mm, tracker = stand_in_modules(overlap=overlap, use_binary_mask_iou=use_binary_mask_iou)

    class Track(StandInTrack):
        def encode_all_masks(self):
            for t in range(len(self.masks)):
                if self.masks[t] is not None and not isinstance(self.masks[t], dict):
                    self.masks[t] = tm.encode_mask(self.masks[t])

        def get_formatted_result(self, video_id):
            return {"video_id": int(video_id), "segmentations": list(self.masks)}

    tm.Track = Track
    return tm, mm, tracker


def stock_bits(maps, size):
    return (F.interpolate(maps.float(), size=tuple(size), mode="bilinear", align_corners=False) > 0).numpy()


def fake_binary_iou(calls):
    """``ops.mask_binary_iou`` by the numpy oracle on torch's own upsample."""
    def mask_binary_iou(a, b, size, *, reduce="volume"):
        calls.append((a, b, tuple(size), reduce))
        return torch.from_numpy(B.iou(*B.counts_of_bits(stock_bits(a, size), stock_bits(b, size)), reduce))
    return mask_binary_iou


def test_process_masks_with_gpu_binary_iou_keeps_the_stitching_frames(monkeypatch):
    import devis_amd
    from devis_amd import ops
    calls = []
    monkeypatch.setattr(ops, "binarize_masks", fake_binarize(calls))
    masks = O.blob_logits(6, 1, 5, 7, 3)[:, 0].float()
    for binary in (True, False):
        tm, mm, tracker = binary_modules(overlap=2, use_binary_mask_iou=binary)
        previous = devis_amd.patch_tracker(tm, mm, gpu_binary_iou=True)
        for start_idx, idx in ((0, 0), (0, 1), (1, 2), (3, 1)):
            calls.clear()
            out = tracker.process_masks(start_idx, idx, (15, 21), masks)
            choice = reference_choice(False, 2, start_idx, idx, 6)         # the soft cost's choice, in binary mode too
            assert [isinstance(m, dict) for m in out] == choice
            assert [isinstance(m, devis_amd.LogitMask) for m in out] == [not c for c in choice]
            assert calls == ([((sum(choice), 5, 7), (15, 21), "F")] if any(choice) else [])
            for t, m in enumerate(out):
                if not choice[t]:
                    assert torch.equal(m.logits, masks[t]) and m.size == (15, 21)
        devis_amd.unpatch_tracker(tm, mm, previous)
        assert tracker.process_masks(0, 0, (15, 21), masks) == "theirs"
    # without the keyword binary mode encodes every frame, as before
    tm, mm, tracker = binary_modules(overlap=2)
    previous = devis_amd.patch_tracker(tm, mm)
    assert all(isinstance(m, dict) for m in tracker.process_masks(0, 0, (15, 21), masks))
    devis_amd.unpatch_tracker(tm, mm, previous)


@pytest.mark.parametrize("reduce", ["volume", "frame"])
def test_binary_cost_is_one_operator_call_on_the_stacked_logits(reduce, monkeypatch):
    import devis_amd
    from devis_amd import ops
    calls, soft_calls = [], []
    monkeypatch.setattr(ops, "mask_binary_iou", fake_binary_iou(calls))
    monkeypatch.setattr(ops, "mask_soft_iou", lambda *a, **k: soft_calls.append(a))
    tm, mm, tracker = binary_modules(overlap=2)
    previous = devis_amd.patch_tracker(tm, mm, gpu_binary_iou=True)
    matcher = tracker.hungarian_matcher
    a, b = O.blob_logits(3, 4, 5, 7, 5).float(), O.blob_logits(4, 3, 5, 7, 6).float()
    size = (15, 21)
    wrap = lambda maps: [devis_amd.LogitMask(m, size) for m in maps]      # noqa: E731
    video = [StandInTrack(i, [None] + wrap(a[i]), last_t=4) for i in range(3)]       # the last two frames before last_t = 4
    clip = [StandInTrack(j, wrap(b[j]), start_idx=1) for j in range(4)]              # the two frames from start_idx = 1
    fn = matcher.compute_volumetric_iou_cost if reduce == "volume" else matcher.compute_frame_average_iou_cost
    cost = fn(video, clip)
    assert len(calls) == 1 and calls[0][2:] == (size, reduce) and soft_calls == []
    assert torch.equal(calls[0][0], a[:, 1:3]) and torch.equal(calls[0][1], b[:, 1:3])
    assert isinstance(cost, np.ndarray) and cost.dtype == np.float64 and cost.shape == (3, 4)
    bits_a, bits_b = stock_bits(a[:, 1:3], size), stock_bits(b[:, 1:3], size)
    reference = B.reference_volume if reduce == "volume" else B.reference_frame
    assert np.array_equal(cost, reference(list(bits_a), list(bits_b))) and cost.max() > 0.05
    assert fn([], clip).shape == (0, 4) and fn(video, []).shape == (3, 0) and len(calls) == 1
    # a frame without a detection is an empty map: zeros, which set no bit
    video[1].masks[3] = None
    clip[2].masks[1] = None
    cost = fn(video, clip)
    assert len(calls) == 2 and tuple(calls[1][0].shape) == (3, 2, 5, 7)
    assert not calls[1][0][1, 1].any() and not calls[1][1][2, 0].any() and torch.equal(calls[1][0][1, 0], a[1, 1])
    wa = [[m for m in w] for w in bits_a]
    wb = [[m for m in w] for w in bits_b]
    wa[1][1], wb[2][0] = None, None
    assert np.array_equal(cost, reference(wa, wb))
    # a window of encodings and None only goes to the replaced method
    rle = {"size": [15, 21], "counts": "x"}
    encoded_video = [StandInTrack(i, [rle, None, rle, rle], last_t=4) for i in range(3)]
    encoded_clip = [StandInTrack(j, [rle, rle, None], start_idx=1) for j in range(4)]
    assert fn(encoded_video, encoded_clip) == "their " + reduce and len(calls) == 2
    # a mixed window raises
    with pytest.raises(TypeError, match="one kind"):
        fn(encoded_video, clip)
    video[0].masks[2] = rle
    with pytest.raises(TypeError, match="one kind"):
        fn(video, clip)
    video[0].masks[2] = torch.zeros(15, 21)
    with pytest.raises(TypeError, match="Tensor"):
        fn(video, clip)
    video[0].masks[2] = devis_amd.LogitMask(a[0, 1], (15, 22))
    with pytest.raises(RuntimeError, match="different sizes"):
        fn(video, clip)
    assert len(calls) == 2
    # soft mode is untouched by the keyword
    matcher.use_binary_mask_iou = False
    video[0].masks[2] = devis_amd.LogitMask(a[0, 1], size)
    video[1].masks[3] = devis_amd.LogitMask(a[1, 2], size)
    clip[2].masks[1] = devis_amd.LogitMask(b[2, 1], size)
    with pytest.raises(AttributeError):
        fn(video, clip)                     # (the stand-in soft operator returned None: it was called)
    assert len(soft_calls) == 1 and len(calls) == 2
    devis_amd.unpatch_tracker(tm, mm, previous)
    assert mm.HungarianInferenceMatcher.compute_volumetric_iou_cost is previous["compute_volumetric_iou_cost"]


def test_get_formatted_result_leaves_no_logit_mask(monkeypatch):
    import devis_amd
    from devis_amd import ops
    monkeypatch.setattr(ops, "binarize_masks", fake_binarize([]))
    tm, mm, tracker = binary_modules(overlap=2)
    theirs = tm.Track.get_formatted_result
    previous = devis_amd.patch_tracker(tm, mm, gpu_binary_iou=True)
    assert tm.Track.get_formatted_result is not theirs and previous["get_formatted_result"] is theirs
    masks = O.blob_logits(6, 1, 5, 7, 3)[:, 0].float()
    track = tm.Track(0, tracker.process_masks(0, 0, (15, 21), masks))
    track.masks[1] = None
    assert sum(isinstance(m, devis_amd.LogitMask) for m in track.masks) == 2
    result = track.get_formatted_result(7)
    assert result["video_id"] == 7 and len(result["segmentations"]) == 6
    assert [type(m) for m in result["segmentations"]] == [dict, type(None), dict, dict, dict, dict]
    assert all(isinstance(m["counts"], str) and m["size"] == [15, 21] for m in result["segmentations"] if m is not None)
    assert len(tm.mask_util.seen) == 6 and np.array_equal(tm.mask_util.seen[-1], stock_bits(masks[None, 5:6], (15, 21))[0, 0])
    devis_amd.unpatch_tracker(tm, mm, previous)
    assert tm.Track.get_formatted_result is theirs


def test_patch_tracker_has_a_fifth_key_with_the_keyword_only_and_restores_all_of_them():
    import devis_amd
    four = {"process_masks", "encode_mask", "compute_volumetric_iou_cost", "compute_frame_average_iou_cost"}
    tm, mm, tracker = binary_modules()
    tm.mask_util.frPyObjects = lambda obj, h, w: {"size": [h, w], "counts": b"packed"}
    now = lambda: (tm.Tracker.process_masks, tm.encode_mask, mm.HungarianInferenceMatcher.compute_volumetric_iou_cost,      # noqa: E731
                   mm.HungarianInferenceMatcher.compute_frame_average_iou_cost, tm.Track.get_formatted_result)
    theirs = now()
    for kw in (dict(), dict(gpu_rle=True)):
        previous = devis_amd.patch_tracker(tm, mm, **kw)
        assert set(previous) == four and now()[4] is theirs[4]
        devis_amd.unpatch_tracker(tm, mm, previous)
        assert now() == theirs
    for kw in (dict(gpu_binary_iou=True), dict(gpu_binary_iou=True, gpu_rle=True)):
        previous = devis_amd.patch_tracker(tm, mm, **kw)
        assert set(previous) == four | {"get_formatted_result"}
        assert tuple(previous[k] for k in ("process_masks", "encode_mask", "compute_volumetric_iou_cost",
                                           "compute_frame_average_iou_cost", "get_formatted_result")) == theirs
        assert all(n is not t for n, t in zip(now(), theirs))
        devis_amd.unpatch_tracker(tm, mm, previous)
        assert now() == theirs
    # a module without Track: refused before anything is replaced; without the keyword it is taken as before
    tm2, mm2, _ = stand_in_modules(use_binary_mask_iou=True)
    before = (tm2.Tracker.process_masks, tm2.encode_mask, mm2.HungarianInferenceMatcher.compute_volumetric_iou_cost)
    with pytest.raises(AttributeError, match="Track"):
        devis_amd.patch_tracker(tm2, mm2, gpu_binary_iou=True)
    assert (tm2.Tracker.process_masks, tm2.encode_mask, mm2.HungarianInferenceMatcher.compute_volumetric_iou_cost) == before
    devis_amd.unpatch_tracker(tm2, mm2, devis_amd.patch_tracker(tm2, mm2))
    with pytest.raises(TypeError):
        devis_amd.patch_tracker(tm, mm, False, True)           # keyword only
    assert isinstance(tm, types.SimpleNamespace) and isinstance(tm.mask_util, StandInMaskUtil)


def test_documents_describe_the_operator():
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Binary mask IoU" in integration and "mask_binary_iou" in integration and "gpu_binary_iou=True" in integration
    assert "pycocotools" in integration and "get_formatted_result" in integration
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^#+ 14\b", design, re.M) and "maskbiou" in design and "mask_bits.h" in design
    for phrase in ("atomic", "conflict", "popcount"):
        assert phrase in design.split(re.search(r"^#+ 14\b", design, re.M).group(0), 1)[1], phrase
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "maskbiou.h" in readme and "mask_binary_iou" in readme and "maskbiou_bench.json" in readme
    import devis_amd
    from devis_amd import argument_builders, ops, tracking
    assert "mask_binary_iou" in ops.__doc__ and "maskbiou.h" in devis_amd.__doc__
    assert "gpu_binary_iou" in argument_builders.patch_tracker.__doc__ and "gpu_binary_iou" in tracking.__doc__
