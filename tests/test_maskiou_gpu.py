"""GPU tests of the clip-stitching operators (include/maskiou.h): the soft IoU matrix against the reference fixtures and the
float64 oracle, the edges of the output blocks, pixel tiles and split ranges, the bitwise promises of the header, memory and
special values, the binarised masks in both layouts, and the patched stand-in tracker and matcher, HIP graphs and
torch.compile.  Tolerance: max|got - want| <= tol * max|want| per tensor, tol = test_attmap_gpu.TOL of the arithmetic type --
1e-4 for float32 arithmetic (bf16 and f16 logits are rounded once before both sides see them, and nothing is stored in 16
bits), 1e-10 for float64."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import maskiou_oracle as O
from conftest import golden, golden_names
from test_attmap_gpu import TOL as ATTMAP_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16]
F64 = torch.float64
FIXTURES = golden_names("maskiou_")


def tol_of(dtype):
    return ATTMAP_TOL[F64] if dtype == F64 else ATTMAP_TOL[torch.float32]


def arith_of(dtype):
    return F64 if dtype == F64 else torch.float32


def assert_close(got, want, tol, what):
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print("%s: max error %.3e, scale %.3e" % (what, err, scale))
    assert err <= tol * scale, (what, err, scale)


def tiles():
    from devis_amd import _maskiou as M
    return {k: M.tile(getattr(M, "TILE_" + k)) for k in ("BLOCK", "ROWS", "COLS", "SPLIT_TILES", "MAX_SPLITS", "BIN_PIXELS", "BIN_SRC")}


def check_all(a, b, size, dtype, what):
    """iou in both modes and the three terms of (a, b) rounded to ``dtype`` against the oracle."""
    import devis_amd
    a, b = a.to(dtype), b.to(dtype)
    tol = tol_of(dtype)
    for reduce in ("volume", "frame"):
        got = devis_amd.mask_soft_iou(a.to(DEV), b.to(DEV), size, reduce=reduce)
        assert got.dtype == arith_of(dtype) and not got.requires_grad
        assert_close(got, O.soft_iou(a, b, size, reduce, arith=arith_of(dtype)), tol, "%s iou %s" % (what, reduce))
    got = devis_amd.mask_soft_iou_terms(a.to(DEV), b.to(DEV), size)
    a4, b4 = (a, b) if a.dim() == 4 else (a[:, None], b[:, None])
    for g, w, name in zip(got, O.terms(a4, b4, size, arith_of(dtype)), ("inter", "sum_a", "sum_b")):
        assert_close(g, w, tol, "%s %s" % (what, name))


# ---- reference and oracle --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_in_float64_equal_the_reference(name):
    import devis_amd
    d = {k: torch.from_numpy(v) for k, v in golden(name).items()}
    size = tuple(int(v) for v in d["size"])
    for reduce in ("volume", "frame"):
        got = devis_amd.mask_soft_iou(d["a"].to(DEV), d["b"].to(DEV), size, reduce=reduce)
        assert got.dtype == F64
        assert_close(got, d["iou_" + reduce], 1e-10, "%s %s" % (name, reduce))
    for side in ("a", "b"):
        bits = devis_amd.binarize_masks(d[side].flatten(0, 1).to(DEV), size).cpu()
        x = O.logits(d[side].flatten(0, 1), size, F64)
        clear = x.abs() > 1e-9          # (exact ties exist in the fixtures: see tests/test_maskiou_cpu.py)
        assert torch.equal(bits[clear], d["bits_" + side].flatten(0, 1)[clear]) and float(clear.double().mean()) > 0.98


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_in_every_dtype_equal_the_oracle(name, dtype):
    d = {k: torch.from_numpy(v) for k, v in golden(name).items()}
    check_all(d["a"], d["b"], tuple(int(v) for v in d["size"]), dtype, name)


# ---- block and split edges -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def block_case():
    """2 * block + 1 maps on each side, three frames, (6, 7) -> (20, 23); the float32-rule terms of the whole, once."""
    n = 2 * tiles()["BLOCK"] + 1
    a, b = O.blob_logits(n, 3, 6, 7, 21).float(), O.blob_logits(n, 3, 6, 7, 22).float()
    return a, b, O.terms(a, b, (20, 23))


def _counts():
    blk = 64        # (asserted against maskiou_tile in the test)
    return [(1, 1, 1), (2, blk - 1, 2), (blk - 1, 2, 3), (blk, blk, 1), (blk + 1, blk, 2), (blk, blk + 1, 3),
            (2 * blk + 1, 1, 1), (1, 2 * blk + 1, 2), (2 * blk + 1, 2 * blk + 1, 3), (blk + 1, 2 * blk + 1, 1)]


@pytest.mark.parametrize("Na,Nb,Fr", _counts())
def test_block_edges(Na, Nb, Fr):
    import devis_amd
    assert tiles()["BLOCK"] == 64
    a, b, (inter, sa, sb) = block_case()
    a, b = a[-Na:, :Fr], b[:Nb, :Fr]            # (the last maps of a: a block's rows are not always the first ones)
    inter, sa, sb = inter[:Fr, -Na:, :Nb], sa[:Fr, -Na:], sb[:Fr, :Nb]
    got = devis_amd.mask_soft_iou_terms(a.to(DEV), b.to(DEV), (20, 23))
    for g, w, name in zip(got, (inter, sa, sb), ("inter", "sum_a", "sum_b")):
        assert_close(g, w, 1e-4, name)
    I, Sa, Sb = inter.sum(0), sa.sum(0), sb.sum(0)
    assert_close(devis_amd.mask_soft_iou(a.to(DEV), b.to(DEV), (20, 23)), I / (Sa[:, None] + Sb[None] - I).clamp(min=1e-6), 1e-4, "volume")
    frame = (inter / (sa[:, :, None] + sb[:, None] - inter).clamp(min=1e-6)).mean(0)
    assert_close(devis_amd.mask_soft_iou(a.to(DEV), b.to(DEV), (20, 23), reduce="frame"), frame, 1e-4, "frame")


def _pixel_cases():
    th, tw, least, most = 2, 16, 4, 128     # (asserted against maskiou_tile in the test)
    tile = th * tw
    return [
        ("one tile - 1", 1, (3, 4), (1, tile - 1)), ("one tile", 1, (3, 4), (th, tw)), ("one tile + 1", 1, (3, 4), (3, 11)),
        ("one tile of two frames", 2, (3, 4), (th, tw // 2)), ("three frames, a tile and a pixel", 3, (3, 4), (1, 11)),
        ("two split ranges + 1 pixel", 1, (2, 9), (th, 2 * least * tw + 1)),
        ("two split ranges + 1 pixel, two frames", 2, (2, 9), (th, 2 * least * tw + 1)),
        ("more tiles than split ranges", 1, (5, 40), (2 * th * 4, tw * (most * least // 8 + 1))),
        ("narrower than a tile row", 1, (4, 3), (9, 5)), ("wider than two tile rows", 2, (4, 9), (5, 2 * tw + 5)),
        ("one source pixel", 2, (1, 1), (5, 7)), ("one source row", 1, (1, 6), (4, 19)), ("one source column", 1, (6, 1), (19, 4)),
        ("the identity", 2, (6, 7), (6, 7)), ("downsampling", 1, (26, 22), (13, 11)), ("one destination pixel", 1, (3, 4), (1, 1)),
    ]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("what,Fr,hw,size", _pixel_cases())
def test_tile_and_split_edges(what, Fr, hw, size, dtype):
    from devis_amd import _maskiou
    t = tiles()
    assert (t["ROWS"], t["COLS"], t["SPLIT_TILES"], t["MAX_SPLITS"]) == (2, 16, 4, 128)
    if what.startswith("two split ranges"):
        assert _maskiou.splits(*size) == (2 * t["SPLIT_TILES"] + 1, t["SPLIT_TILES"], 3)
    if what == "more tiles than split ranges":
        assert _maskiou.splits(*size)[1] == t["SPLIT_TILES"] + 1
    a, b = O.blob_logits(3, Fr, hw[0], hw[1], 31), O.blob_logits(5, Fr, hw[0], hw[1], 32)
    check_all(a, b, size, dtype, what)


def test_three_dimensional_inputs_are_one_frame():
    import devis_amd
    a, b = O.blob_logits(3, 1, 6, 7, 41).float(), O.blob_logits(4, 1, 6, 7, 42).float()
    one = devis_amd.mask_soft_iou(a[:, 0].to(DEV), b[:, 0].to(DEV), (20, 23))
    assert torch.equal(one, devis_amd.mask_soft_iou(a.to(DEV), b.to(DEV), (20, 23)))
    check_all(a[:, 0], b[:, 0], (20, 23), torch.float32, "three-dimensional")


def test_non_dense_inputs_and_no_maps():
    import devis_amd
    a, b = O.blob_logits(3, 2, 6, 14, 43).float().to(DEV), O.blob_logits(4, 2, 6, 7, 44).float().to(DEV)
    strided = a[:, :, :, ::2]
    assert not strided.is_contiguous()
    assert torch.equal(devis_amd.mask_soft_iou(strided, b, (20, 23)), devis_amd.mask_soft_iou(strided.contiguous(), b, (20, 23)))
    full = devis_amd.mask_soft_iou_terms(strided, b, (20, 23))
    inter, sa, sb = devis_amd.mask_soft_iou_terms(strided[:0], b, (20, 23))
    assert tuple(inter.shape) == (2, 0, 4) and tuple(sa.shape) == (2, 0) and torch.equal(sb, full[2])
    inter, sa, sb = devis_amd.mask_soft_iou_terms(strided, b[:0], (20, 23))
    assert tuple(inter.shape) == (2, 3, 0) and tuple(sb.shape) == (2, 0) and torch.equal(sa, full[1])
    assert tuple(devis_amd.mask_soft_iou(strided[:0], b[:0], (20, 23)).shape) == (0, 0)
    assert tuple(devis_amd.binarize_masks(b[:0, 0], (20, 23)).shape) == (0, 20, 23)


# ---- bitwise ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
def test_bitwise_promises(dtype):
    import devis_amd
    n = tiles()["BLOCK"] + 6
    size = (20, 2 * tiles()["SPLIT_TILES"] * tiles()["COLS"] + 3)       # several split ranges
    a, b = O.blob_logits(n, 2, 6, 7, 51).to(dtype).to(DEV), O.blob_logits(n, 2, 6, 7, 52).to(dtype).to(DEV)
    iou = devis_amd.mask_soft_iou(a, b, size)
    inter, sa, sb = devis_amd.mask_soft_iou_terms(a, b, size)
    # two runs
    assert torch.equal(iou, devis_amd.mask_soft_iou(a, b, size)) and torch.equal(inter, devis_amd.mask_soft_iou_terms(a, b, size)[0])
    # any sub-block alone: inside the first block, across the block edge, one entry
    for ra, rb in ((slice(3, 5), slice(60, 70)), (slice(62, 67), slice(0, 3)), (slice(69, 70), slice(1, 2))):
        sub = devis_amd.mask_soft_iou_terms(a[ra], b[rb], size)
        assert torch.equal(sub[0], inter[:, ra, rb]) and torch.equal(sub[1], sa[:, ra]) and torch.equal(sub[2], sb[:, rb])
        assert torch.equal(devis_amd.mask_soft_iou(a[ra], b[rb], size), iou[ra, rb])
        assert torch.equal(devis_amd.mask_soft_iou(a[ra], b[rb], size, reduce="frame"), devis_amd.mask_soft_iou(a, b, size, reduce="frame")[ra, rb])
    # the transpose, on operands that are not each other's mirror
    back = devis_amd.mask_soft_iou_terms(b, a, size)
    assert torch.equal(back[0].transpose(1, 2), inter) and torch.equal(back[1], sb) and torch.equal(back[2], sa)
    assert not torch.equal(inter, inter.transpose(1, 2))
    assert torch.equal(devis_amd.mask_soft_iou(b, a, size).t(), iou)
    # a map's sum alone and in the batch, as a and as b
    alone = devis_amd.mask_soft_iou_terms(a[7:8], a[7:8], size)
    assert torch.equal(alone[1], sa[:, 7:8]) and torch.equal(alone[2], sa[:, 7:8])
    # the same logits at an odd storage offset and 16-byte aligned
    base = torch.empty(a.numel() + 1, dtype=dtype, device=DEV)
    odd = base[1:].view(a.shape).copy_(a)
    assert odd.data_ptr() % 16 != 0 and a.data_ptr() % 16 == 0
    assert torch.equal(devis_amd.mask_soft_iou(odd, b, size), iou) and torch.equal(devis_amd.mask_soft_iou(b, odd, size).t(), iou)
    bits = devis_amd.binarize_masks(a[:, 0], size)
    assert torch.equal(devis_amd.binarize_masks(odd[:, 0], size), bits)


# ---- memory and special values -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("Na,Nb", [(3, 5), (65, 2)])
def test_outputs_and_workspace_prefilled_with_nan_come_back_written(Na, Nb, dtype):
    from devis_amd import _maskiou, _native
    size = (9, 2 * tiles()["SPLIT_TILES"] * tiles()["COLS"] + 1)
    a, b = O.blob_logits(Na, 2, 4, 5, 61).to(dtype).to(DEV), O.blob_logits(Nb, 2, 4, 5, 62).to(dtype).to(DEV)
    shape = _maskiou.Shape(Na, Nb, 2, 4, 5, size[0], size[1])
    code = _native.dtype_code(dtype)
    nan = lambda *s: torch.full(s, float("nan"), dtype=dtype, device=DEV)      # noqa: E731
    ws = nan(_maskiou.workspace_bytes(code, shape) // a.element_size())
    outs = nan(2, Na, Nb), nan(2, Na), nan(2, Nb), nan(Na, Nb)
    _maskiou.pairwise(code, _maskiou.VOLUME, a, b, shape, 1e-6, ws.view(torch.uint8), outs[0], outs[1], outs[2], outs[3])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    want = O.terms(a.cpu(), b.cpu(), size, dtype)
    for g, w, name in zip(outs[:3], want, ("inter", "sum_a", "sum_b")):
        assert_close(g, w, tol_of(dtype), name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_saturated_and_infinite_logits(dtype):
    import devis_amd
    inf = float("inf")
    size, P = (11, 19), 11 * 19
    maps = torch.zeros(6, 1, 4, 5)
    maps[0], maps[1], maps[2], maps[3] = 100.0, -100.0, inf, -inf
    maps[4] = O.blob_logits(1, 1, 4, 5, 71)[0].float()
    maps[5] = maps[4]
    maps[5, 0, :2, :2] = inf            # an infinite blob on a finite map: +inf or finite everywhere, never NaN
    x = maps.to(dtype).to(DEV)
    for reduce in ("volume", "frame"):
        iou = devis_amd.mask_soft_iou(x, x, size, reduce=reduce).double().cpu()
        assert bool(torch.isfinite(iou).all())
        ones = iou[[0, 2]][:, [0, 2]]
        assert float((ones - 1).abs().max()) <= 1e-6                        # p = 1 everywhere: I = U = P
        assert float(iou[[1, 3]].abs().max()) <= 1e-30 and float(iou[:, [1, 3]].abs().max()) <= 1e-30     # p = 0 (or 4e-44)
    inter, sa, sb = devis_amd.mask_soft_iou_terms(x, x, size)
    assert bool(torch.isfinite(inter).all()) and torch.equal(sa, sb)
    assert float(sa[0, 2]) == P and float(sa[0, 0]) == P and float(sa[0, 3]) == 0.0
    assert float(sa[0, 5]) >= float(sa[0, 4])
    bits = devis_amd.binarize_masks(x[:, 0], size).cpu()
    assert bool(bits[0].all()) and bool(bits[2].all()) and not bool(bits[1].any()) and not bool(bits[3].any())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_a_nan_poisons_its_own_row_or_column_only(dtype):
    import devis_amd
    a, b = O.blob_logits(4, 2, 6, 7, 81).to(dtype), O.blob_logits(5, 2, 6, 7, 82).to(dtype)
    a[2, 0, 3, 3] = float("nan")
    b[1, 1, 0, 0] = float("nan")
    for reduce in ("volume", "frame"):
        iou = devis_amd.mask_soft_iou(a.to(DEV), b.to(DEV), (20, 23), reduce=reduce).cpu()
        bad = torch.zeros(4, 5, dtype=torch.bool)
        bad[2, :], bad[:, 1] = True, True
        assert torch.equal(torch.isnan(iou), bad)
    inter, sa, sb = (t.cpu() for t in devis_amd.mask_soft_iou_terms(a.to(DEV), b.to(DEV), (20, 23)))
    want = torch.zeros(2, 4, 5, dtype=torch.bool)
    want[0, 2, :], want[1, :, 1] = True, True
    assert torch.equal(torch.isnan(inter), want)
    assert torch.equal(torch.isnan(sa), want[:, :, 0]) and torch.equal(torch.isnan(sb), want[:, 0, :])
    bits = devis_amd.binarize_masks(a[:, 0].to(DEV), (20, 23)).cpu()
    # the pixels the NaN reaches: those with a tap of nonzero weight on it (the oracle's matrix product spreads it further)
    mark = torch.zeros(1, 6, 7, dtype=F64)
    mark[0, 3, 3] = 1.0
    hit = O.logits(mark, (20, 23), arith_of(dtype))[0] > 0
    assert 4 <= int(hit.sum()) < 20 * 23 // 4 and not bool(bits[2][hit].any())                 # NaN gives 0
    clean = a[:, 0].clone()
    clean[2, 3, 3] = 0.0
    want, x = O.binarize(clean, (20, 23), arith_of(dtype))
    keep = ~O.near_zero(x, clean)
    keep[2] &= ~hit
    assert torch.equal(bits[keep], want[keep])


def test_peak_allocation_is_outputs_and_workspace():
    import devis_amd
    from devis_amd import _maskiou
    Na, Nb, Fr, size = 4, 4, 2, (180, 320)
    a, b = O.blob_logits(Na, Fr, 12, 20, 91).float().to(DEV), O.blob_logits(Nb, Fr, 12, 20, 92).float().to(DEV)
    devis_amd.mask_soft_iou(a, b, size)            # the library is loaded, the kernels are resident
    up = lambda n: (n + 511) // 512 * 512      # noqa: E731  (the caching allocator's granule)
    outputs = sum(up(4 * n) for n in (Na * Nb, Fr * Na * Nb, Fr * Na, Fr * Nb))
    workspace = up(_maskiou.workspace_bytes(0, _maskiou.Shape(Na, Nb, Fr, 12, 20, size[0], size[1])))
    for maps, copies in ((a, 0), (torch.cat([a, a], 3)[:, :, :, ::2], up(a.numel() * 4))):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = devis_amd.mask_soft_iou(maps, b, size)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        print("peak %d, outputs %d, workspace %d, copies %d" % (peak, outputs, workspace, copies))
        assert peak <= outputs + workspace + copies
        assert outputs + workspace + copies < size[0] * size[1] * 4          # less than one map of H*W floats
        del out
    src = a[:, 0].contiguous()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    bits = devis_amd.binarize_masks(src, size)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before <= up(Na * size[0] * size[1]) and bits.element_size() == 1


# ---- binarise --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("index", range(len(O.BINARIZE_CASES)))
def test_binarize_equals_the_oracle_outside_the_pixels_near_zero(index, order, dtype):
    import devis_amd
    src, size = O.binarize_case(index, dtype)
    want, x = O.binarize(src, size, arith_of(dtype))
    out = O.near_zero(x, src)
    share = float(out.double().mean())
    got = devis_amd.binarize_masks(src.to(DEV), size, order=order)
    assert got.dtype == torch.bool and tuple(got.shape) == (3,) + size and not got.requires_grad
    if order == "F":
        assert got.stride() == (size[0] * size[1], 1, size[0]) and got.transpose(1, 2).is_contiguous()
    else:
        assert got.is_contiguous()
    got = got.cpu()
    ones = float(want[~out].double().mean())
    print("left out %.2e of the pixels, ones %.3f, differing inside %d" % (share, ones, int((got != want)[out].sum())))
    assert share <= O.BINARIZE_CAP and 0.05 < ones < 0.95
    assert torch.equal(got[~out], want[~out])
    assert (size[0] * size[1]) % 16 != 0 or index == 0
    if index == 4:
        assert min(src.shape[1] * src.shape[2], src.shape[2] * src.shape[1]) > tiles()["BIN_SRC"]      # not staged
    assert got.view(torch.uint8).max() <= 1


@pytest.mark.parametrize("layout", ["row", "col"])
def test_binarize_raw_call_into_a_byte_buffer_at_an_odd_address(layout):
    import devis_amd
    from devis_amd import _maskiou
    src, size = O.binarize_case(0)
    src = src.to(DEV)
    n = 3 * size[0] * size[1]
    buf = torch.full((n + 64,), 7, dtype=torch.uint8, device=DEV)
    out = buf[17:17 + n]
    assert out.data_ptr() % 2 == 1
    code = _maskiou.ROW_MAJOR if layout == "row" else _maskiou.COL_MAJOR
    _maskiou.binarize(0, code, src, 3, src.shape[1], src.shape[2], size[0], size[1], out)
    torch.cuda.synchronize()
    assert bool((buf[:17] == 7).all()) and bool((buf[17 + n:] == 7).all())         # nothing outside
    want = devis_amd.binarize_masks(src, size, order="C" if layout == "row" else "F")
    want = want if layout == "row" else want.transpose(1, 2)
    assert want.is_contiguous() and torch.equal(out.view(want.shape), want.view(torch.uint8))
    # a tile boundary inside a mask, and a mask that does not end on 16 bytes
    big = (67, tiles()["BIN_PIXELS"] // 64 + 3)
    got = devis_amd.binarize_masks(src, big, order="C" if layout == "row" else "F").cpu()
    bits, x = O.binarize(src.cpu(), big)
    keep = ~O.near_zero(x, src.cpu())
    assert torch.equal(got[keep], bits[keep]) and float(keep.double().mean()) >= 1 - O.BINARIZE_CAP


# ---- integration -----------------------------------------------------------------------------------------------------

def test_patched_tracker_and_matcher_end_to_end():
    import devis_amd
    from test_maskiou_cpu import StandInTrack, stand_in_modules, stock_soft_iou
    tm, mm, tracker = stand_in_modules(overlap=2)
    previous = devis_amd.patch_tracker(tm, mm)
    try:
        size = (45, 80)
        clip_a, clip_b = O.blob_logits(4, 5, 12, 20, 101).float().to(DEV), O.blob_logits(3, 5, 12, 20, 102).float().to(DEV)
        # the first clip keeps its last two frames, the second its first two (start_idx 0) and its last two
        video = [StandInTrack(i, tracker.process_masks(0, 0, size, clip_a[i]), last_t=5) for i in range(4)]
        clip = [StandInTrack(j, tracker.process_masks(0, 1, size, clip_b[j])) for j in range(3)]
        assert [isinstance(m, dict) for m in video[0].masks] == [True, True, True, False, False]
        assert [isinstance(m, dict) for m in clip[0].masks] == [False, False, True, False, False]
        seen = tm.mask_util.seen
        assert len(seen) == 4 * 3 + 3 * 1 and all(s.shape == size and s.flags["F_CONTIGUOUS"] for s in seen)
        x = F.interpolate(clip_a[0][:, None].double(), size=size, mode="bilinear", align_corners=False)[:, 0].cpu()
        for t in range(3):
            far = x[t].abs() > 1e-4
            assert np.array_equal(seen[t][far.numpy()], (x[t] > 0).numpy()[far.numpy()])
        matcher = tracker.hungarian_matcher
        for fn, reduce in ((matcher.compute_volumetric_iou_cost, "volume"), (matcher.compute_frame_average_iou_cost, "frame")):
            cost = fn(video, clip)
            assert isinstance(cost, np.ndarray) and cost.dtype == np.float64 and cost.shape == (4, 3)
            want = stock_soft_iou(clip_a[:, 3:].double().cpu(), clip_b[:, :2].double().cpu(), size, reduce)
            assert_close(torch.from_numpy(cost), want, 1e-4, "stitching cost " + reduce)
        rle = tm.encode_mask(video[0].masks[3])
        assert rle["size"] == list(size) and isinstance(rle["counts"], str) and len(seen) == 16
    finally:
        devis_amd.unpatch_tracker(tm, mm, previous)


def test_hip_graph_replay_with_changed_inputs_gives_the_changed_result():
    import devis_amd
    size = (45, 96)
    a, b = O.blob_logits(5, 2, 12, 20, 111).float().to(DEV), O.blob_logits(4, 2, 12, 20, 112).float().to(DEV)
    call = lambda u, v: (devis_amd.mask_soft_iou(u, v, size), devis_amd.binarize_masks(u[:, 0], size, order="F"))      # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(a, b)          # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        iou, bits = call(a, b)
    a2 = O.blob_logits(5, 2, 12, 20, 113).float().to(DEV)
    a.copy_(a2)
    graph.replay()
    torch.cuda.synchronize()
    want_iou, want_bits = call(a2, b)
    assert torch.equal(iou, want_iou) and torch.equal(bits, want_bits)
    assert_close(iou, O.soft_iou(a2.cpu(), b.cpu(), size), 1e-4, "graph replay")


def test_compile_fullgraph_equals_eager_also_with_dynamic_shapes():
    import devis_amd

    def fn(u, v):
        return devis_amd.mask_soft_iou(u, v, (27, 35), reduce="frame"), devis_amd.binarize_masks(u[:, 0], (27, 35), order="F")

    compiled = torch.compile(fn, fullgraph=True, dynamic=True)
    for n in (3, 5):
        a, b = O.blob_logits(n, 2, 7, 9, 120 + n).float().to(DEV), O.blob_logits(n + 1, 2, 7, 9, 130 + n).float().to(DEV)
        got, want = compiled(a, b), fn(a, b)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[1].stride() == want[1].stride()
