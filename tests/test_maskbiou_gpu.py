"""GPU tests of the binary mask IoU (include/maskbiou.h): the counts against chosen bit patterns at the edges of the packed
words, of the LDS chunks, of the split ranges and of the pair blocks, against ``binarize_masks`` at every pixel and against the
independent oracle, a larger case, the two ratios, independence of batch, workspace, strides and run, special values, memory,
HIP graphs and torch.compile, and the stand-in tracker patched with ``gpu_binary_iou=True``.  Everything is integers: every
comparison of counts is exact, and a ratio is compared with ``==``."""
import functools

import numpy as np
import pytest
import torch

import maskbiou_oracle as B
import maskiou_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16]
F64 = torch.float64


def arith_of(dtype):
    return F64 if dtype == F64 else torch.float32


def tiles():
    from devis_amd import _maskbiou as M
    return {k: M.tile(getattr(M, "TILE_" + k)) for k in ("BLOCK", "CHUNK_WORDS", "SPLIT_WORDS")}


def terms(a, b, size):
    """The operator's counts as numpy int64, after checking their shapes and dtypes."""
    import devis_amd
    inter, area_a, area_b = devis_amd.mask_binary_iou_terms(a, b, size)
    Na, Nb, F = a.shape[0], b.shape[0], a.shape[1]
    assert tuple(inter.shape) == (Na, Nb, F) and tuple(area_a.shape) == (Na, F) and tuple(area_b.shape) == (Nb, F)
    for t in (inter, area_a, area_b):
        assert t.dtype == torch.int32 and t.is_contiguous() and not t.requires_grad and t.device == a.device
    return tuple(t.cpu().numpy().astype(np.int64) for t in (inter, area_a, area_b))


def binarized(src, size):
    """``binarize_masks`` of [N, F, h, w] logits as numpy bool [N, F, H, W]."""
    import devis_amd
    N, F = src.shape[:2]
    return devis_amd.binarize_masks(src.flatten(0, 1), size).view(N, F, *size).cpu().numpy()


def torch_counts(a, b, size):
    """The counts torch forms on the device from ``binarize_masks`` (a float64 product of 0/1 maps: exact below 2^53)."""
    import devis_amd
    A = devis_amd.binarize_masks(a.flatten(0, 1), size).view(a.shape[0], a.shape[1], -1).double()
    Bm = devis_amd.binarize_masks(b.flatten(0, 1), size).view(b.shape[0], b.shape[1], -1).double()
    inter = torch.einsum("ifk,jfk->ijf", A, Bm)
    return tuple(t.round().long().cpu().numpy() for t in (inter, A.sum(2), Bm.sum(2)))


def assert_equal_counts(got, want, note=None):
    for name, g, w in zip(("inter", "area_a", "area_b"), got, want):
        assert np.array_equal(g, w), (name, note, np.argwhere(g != w)[:4].tolist())


# ---- exact bit patterns ----------------------------------------------------------------------------------------------

def _pattern_sizes():
    C, S = 32, 256          # words per chunk and per split range (asserted against maskbiou_tile in the test)
    sizes = [(1, 1), (8, 8), (5, 13), (67, 61)]
    for words in (C - 1, C, C + 1, S - 1, S, S + 1):
        sizes.append((64, words))           # P = 64 * words: exactly that many full words
    sizes += [(1, 64 * C + 1), (3, (64 * S + 1) // 3 + 1), (7, 64 * 2 * S // 7)]     # a bit into the next chunk / split range
    return sizes


def _walks(P, g):
    """(name, walk [P] bool): masks given by their column-major walk."""
    q = np.arange(P)
    return [("half", g.random(P) < 0.5), ("sparse", g.random(P) < 0.05), ("zeros", q < 0), ("ones", q >= 0),
            ("checker from 1", q % 2 == 0), ("checker from 0", q % 2 == 1), ("pixel 0", q == 0), ("pixel P-1", q == P - 1),
            ("half again", g.random(P) < 0.5), ("alternating words", (q // 64) % 2 == 0)]


@pytest.mark.parametrize("H,W", _pattern_sizes())
def test_exact_bit_patterns_through_an_identity_resample(H, W):
    import devis_amd
    t = tiles()
    assert (t["CHUNK_WORDS"], t["SPLIT_WORDS"]) == (32, 256)
    P = H * W
    g = np.random.default_rng(H * 1000 + W)
    names, walks = zip(*_walks(P, g))
    n = len(walks)
    # track i of a: patterns i, i + 1, i + 2 in its F = 3 frames; track j of b: j + 3, j + 5, j + 7
    pick = lambda offs: np.stack([np.stack([walks[(i + o) % n].reshape(W, H).T for o in offs]) for i in range(n)])      # noqa: E731
    bits_a, bits_b = pick((0, 1, 2)), pick((3, 5, 7))[:n - 3]                  # [10, 3, H, W] and [7, 3, H, W]
    to_logits = lambda bits: torch.from_numpy(np.where(bits, 1.0, -1.0).astype(np.float32)).to(DEV)      # noqa: E731
    a, b = to_logits(bits_a), to_logits(bits_b)
    assert np.array_equal(binarized(a, (H, W)), bits_a)                        # the bits are chosen, not computed
    want = B.counts_of_bits(bits_a, bits_b)
    assert_equal_counts(terms(a, b, (H, W)), want)
    assert want[1][:, 0].tolist()[2:4] == [0, P] and want[1][6, 0] == 1 and want[1][7, 0] == 1
    for F in (1, 2):
        assert_equal_counts(terms(a[:, :F], b[:, :F], (H, W)), tuple(w[..., :F] for w in want), F)
    if (H, W) in ((5, 13), (64, 257)):      # the other storage types (+1 and -1 are exact in each), and the ratios
        for dtype in (F64, torch.bfloat16, torch.float16):
            assert_equal_counts(terms(a.to(dtype), b.to(dtype), (H, W)), want, dtype)
        for reduce in ("volume", "frame"):
            got = devis_amd.mask_binary_iou(a, b, (H, W), reduce=reduce).cpu().numpy()
            assert np.array_equal(got, B.iou(*want, reduce))


@functools.lru_cache(maxsize=None)
def block_case():
    """Random bits at 9 x 15 (P = 135: three words, the last with 7 bits) for block + 1 tracks a side."""
    g = np.random.default_rng(77)
    n = tiles()["BLOCK"] + 1
    bits_a, bits_b = g.random((n, 3, 9, 15)) < 0.5, g.random((n, 3, 9, 15)) < 0.2
    bits_a[1], bits_b[2] = False, True
    return bits_a, bits_b, B.counts_of_bits(bits_a, bits_b)


def _block_counts():
    block = 32
    return [(1, block - 1), (block - 1, block), (block, block + 1), (block + 1, 1), (block, 1), (block + 1, block - 1)]


@pytest.mark.parametrize("F", [1, 2, 3])
@pytest.mark.parametrize("Na,Nb", _block_counts())
def test_numbers_of_tracks_around_the_pair_block(Na, Nb, F):
    assert tiles()["BLOCK"] == 32 and Na != Nb
    bits_a, bits_b, want = block_case()
    a = torch.from_numpy(np.where(bits_a[:Na, :F], 1.0, -1.0).astype(np.float32)).to(DEV)
    b = torch.from_numpy(np.where(bits_b[:Nb, :F], 1.0, -1.0).astype(np.float32)).to(DEV)
    assert_equal_counts(terms(a, b, (9, 15)), (want[0][:Na, :Nb, :F], want[1][:Na, :F], want[2][:Nb, :F]))


# ---- binarise and the oracle ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("index", range(len(O.BINARIZE_CASES)))
def test_counts_are_those_of_binarize_masks_and_of_the_oracle_up_to_near_zero_pixels(index, dtype):
    src, size = O.binarize_case(index, dtype)                  # the inputs whose near-zero share the CPU suite caps
    a, b = src[:2, None], src[1:, None]                         # [2, 1, h, w] each; they share a map
    got = terms(a.to(DEV), b.to(DEV), size)
    assert_equal_counts(got, torch_counts(a.to(DEV), b.to(DEV), size))          # every pixel, without exception
    assert_equal_counts(got, B.counts_of_bits(binarized(a.to(DEV), size), binarized(b.to(DEV), size)))
    # the independent oracle: a count differs by at most the near-zero pixels of the masks involved
    want = B.counts(a, b, size, arith_of(dtype))
    _, x = O.binarize(src, size, arith_of(dtype))
    near = O.near_zero(x, src).flatten(1).sum(1).numpy()                        # per map of src
    near_a, near_b = near[:2, None], near[1:, None]
    assert float(near.sum()) <= O.BINARIZE_CAP * x.numel()
    assert (np.abs(got[1] - want[1]) <= near_a).all() and (np.abs(got[2] - want[2]) <= near_b).all()
    assert (np.abs(got[0] - want[0]) <= near_a[:, None, :] + near_b[None, :, :]).all()
    assert got[0].max() > 0 and 0.05 < got[1].mean() / (size[0] * size[1]) < 0.95


@functools.lru_cache(maxsize=None)
def larger_case():
    return O.blob_logits(33, 2, 45, 80, 301).float(), O.blob_logits(35, 2, 45, 80, 302).float(), (180, 320)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_larger_case_over_several_pair_blocks_and_split_ranges(dtype):
    import devis_amd
    a, b, size = larger_case()
    a, b = a.to(dtype).to(DEV), b.to(dtype).to(DEV)
    t = tiles()
    assert a.shape[0] > t["BLOCK"] and b.shape[0] > t["BLOCK"] and size[0] * size[1] > 3 * 64 * t["SPLIT_WORDS"]
    got = terms(a, b, size)
    want = torch_counts(a, b, size)
    assert_equal_counts(got, want)
    iou = B.iou(*got, "volume")
    assert iou.max() > 0.6 and iou.min() < 0.01 and int(((iou > 0.05) & (iou < 0.6)).sum()) >= 20       # the IoUs spread
    for reduce in ("volume", "frame"):
        assert np.array_equal(devis_amd.mask_binary_iou(a, b, size, reduce=reduce).cpu().numpy(), B.iou(*got, reduce))


# ---- the ratios ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reduce", ["volume", "frame"])
def test_the_ratio_is_the_oracles_of_the_operators_terms_and_the_references_on_the_decoded_bits(reduce):
    import devis_amd
    size = (45, 80)
    a, b = O.blob_logits(5, 3, 12, 20, 311).float(), O.blob_logits(4, 3, 12, 20, 312).float()
    a[1, 2], b[2] = -1.0, -3.0                  # an empty frame, and a track without a set pixel
    a, b = a.to(DEV), b.to(DEV)
    got = devis_amd.mask_binary_iou(a, b, size, reduce=reduce)
    assert got.dtype == F64 and tuple(got.shape) == (5, 4) and got.is_contiguous() and not got.requires_grad
    got = got.cpu().numpy()
    counts = terms(a, b, size)
    assert np.array_equal(got, B.iou(*counts, reduce))
    bits_a, bits_b = binarized(a, size), binarized(b, size)
    reference = B.reference_volume if reduce == "volume" else B.reference_frame
    assert np.array_equal(got, reference(list(bits_a), list(bits_b)))
    assert (got[:, 2] == 0.0).all() and got.max() > 0.2 and ((got >= 0) & (got <= 1)).all()
    if reduce == "volume":      # a frame without a detection in the reference's loop is the empty frame here
        windows = [list(w) for w in bits_a]
        assert not bits_a[1, 2].any()
        windows[1][2] = None
        assert np.array_equal(got, B.reference_volume(windows, list(bits_b)))
    assert np.array_equal(devis_amd.mask_binary_iou(a, b, size).cpu().numpy(), B.iou(*counts, "volume"))       # the default


# ---- independence ----------------------------------------------------------------------------------------------------

def test_counts_do_not_depend_on_workspace_outputs_batch_run_or_strides():
    import devis_amd
    from devis_amd import _maskbiou
    size = (67, 123)
    H, W = size
    a, b = O.blob_logits(7, 2, 9, 14, 321).float().to(DEV), O.blob_logits(5, 2, 9, 14, 322).float().to(DEV)
    first = devis_amd.mask_binary_iou_terms(a, b, size)
    again = devis_amd.mask_binary_iou_terms(a, b, size)
    assert all(torch.equal(x, y) for x, y in zip(first, again))                                 # run to run
    assert_equal_counts(tuple(t.cpu().numpy() for t in first), torch_counts(a, b, size))
    # stale memory: workspace and outputs full of 0x7f bytes; nothing is written outside them
    nbytes = _maskbiou.workspace_bytes(7, 5, 2, H, W)
    ws = torch.full((nbytes + 64,), 0x7f, dtype=torch.uint8, device=DEV)
    buf = torch.full((7 * 5 * 2 + 7 * 2 + 5 * 2 + 48,), 0x7f7f7f7f, dtype=torch.int32, device=DEV)
    inter, area_a, area_b = buf[16:86], buf[86:100], buf[100:110]
    _maskbiou.counts(0, a, b, 7, 5, 2, 9, 14, H, W, ws, inter, area_a, area_b)
    torch.cuda.synchronize()
    assert torch.equal(inter.view(7, 5, 2), first[0]) and torch.equal(area_a.view(7, 2), first[1])
    assert torch.equal(area_b.view(5, 2), first[2])
    assert bool((buf[:16] == 0x7f7f7f7f).all()) and bool((buf[110:] == 0x7f7f7f7f).all()) and bool((ws[-64:] == 0x7f).all())
    # a track alone against a batch, a pair alone, a slice
    for i in (0, 3, 6):
        alone = devis_amd.mask_binary_iou_terms(a[i:i + 1], b, size)
        assert torch.equal(alone[0], first[0][i:i + 1]) and torch.equal(alone[1], first[1][i:i + 1]) and torch.equal(alone[2], first[2])
        pair = devis_amd.mask_binary_iou_terms(a[i:i + 1], b[2:3], size)
        assert torch.equal(pair[0], first[0][i:i + 1, 2:3]) and torch.equal(pair[2], first[2][2:3])
    part = devis_amd.mask_binary_iou_terms(a[2:5], b[1:4], size)
    assert torch.equal(part[0], first[0][2:5, 1:4]) and torch.equal(part[1], first[1][2:5]) and torch.equal(part[2], first[2][1:4])
    # views that are not dense, and logits at an address that is no multiple of 16 bytes
    wide = torch.stack([a, -a], 4).flatten(3)           # [7, 2, 9, 28]: a in the even columns
    view = wide[..., ::2]
    swapped = b.transpose(0, 1).contiguous().transpose(0, 1)          # b in [F, N, h, w] memory
    assert not view.is_contiguous() and torch.equal(view, a) and not swapped.is_contiguous()
    got = devis_amd.mask_binary_iou_terms(view, swapped, size)
    assert all(torch.equal(x, y) for x, y in zip(got, first))
    base = torch.empty(a.numel() + 1, dtype=a.dtype, device=DEV)
    odd = base[1:].view(a.shape).copy_(a)
    assert odd.data_ptr() % 16 != 0
    assert all(torch.equal(x, y) for x, y in zip(devis_amd.mask_binary_iou_terms(odd, b, size), first))


def test_no_maps_on_a_side_gives_empty_outputs():
    import devis_amd
    size = (27, 35)
    a, b = O.blob_logits(3, 2, 7, 9, 331).float().to(DEV), O.blob_logits(4, 2, 7, 9, 332).float().to(DEV)
    full = devis_amd.mask_binary_iou_terms(a, b, size)
    inter, area_a, area_b = devis_amd.mask_binary_iou_terms(a[:0], b, size)
    assert tuple(inter.shape) == (0, 4, 2) and tuple(area_a.shape) == (0, 2) and torch.equal(area_b, full[2])
    inter, area_a, area_b = devis_amd.mask_binary_iou_terms(a, b[:0], size)
    assert tuple(inter.shape) == (3, 0, 2) and tuple(area_b.shape) == (0, 2) and torch.equal(area_a, full[1])
    inter, area_a, area_b = devis_amd.mask_binary_iou_terms(a[:0], b[:0], size)
    assert tuple(inter.shape) == (0, 0, 2) and inter.dtype == area_a.dtype == area_b.dtype == torch.int32
    for reduce in ("volume", "frame"):
        assert tuple(devis_amd.mask_binary_iou(a[:0], b, size, reduce=reduce).shape) == (0, 4)
        assert tuple(devis_amd.mask_binary_iou(a, b[:0], size, reduce=reduce).shape) == (3, 0)
        assert devis_amd.mask_binary_iou(a[:0], b[:0], size, reduce=reduce).dtype == F64


# ---- special values --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_logits_give_the_bits_of_binarize_masks(dtype):
    inf, nan = float("inf"), float("nan")
    size = (11, 19)
    maps = torch.zeros(8, 4, 5)
    maps[0], maps[1], maps[2], maps[3] = inf, -inf, nan, 100.0
    maps[4] = O.blob_logits(1, 1, 4, 5, 71)[0, 0].float()
    maps[5] = maps[4]
    maps[5, :2, :2] = inf                   # an infinite blob on a finite map
    maps[6] = maps[4]
    maps[6, 2, 2] = nan                     # a NaN logit
    maps[7] = -maps[4]
    src = maps.to(dtype).to(DEV)
    a, b = src.view(4, 2, 4, 5), src.flip(0).view(4, 2, 4, 5)
    got = terms(a, b, size)
    assert_equal_counts(got, B.counts_of_bits(binarized(a, size), binarized(b, size)))


# ---- memory ----------------------------------------------------------------------------------------------------------

def test_peak_allocation_is_outputs_and_workspace_and_less_than_one_byte_map():
    import devis_amd
    from devis_amd import _maskbiou
    Na, Nb, F, size = 6, 5, 2, (360, 640)
    H, W = size
    a, b = O.blob_logits(Na, F, 90, 160, 341).float().to(DEV), O.blob_logits(Nb, F, 90, 160, 342).float().to(DEV)
    devis_amd.mask_binary_iou_terms(a[:1], b[:1], (45, 80))           # the library is loaded, the kernels are resident
    up = lambda n: (n + 511) // 512 * 512      # noqa: E731  (the caching allocator's granule)
    outputs = up(4 * Na * Nb * F) + up(4 * Na * F) + up(4 * Nb * F)
    workspace = up(_maskbiou.workspace_bytes(Na, Nb, F, H, W))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = devis_amd.mask_binary_iou_terms(a, b, size)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak %d, outputs %d, workspace %d, byte map of one operand %d" % (peak, outputs, workspace, Na * F * H * W))
    assert peak <= outputs + workspace < min(Na, Nb) * F * H * W
    assert workspace <= (Na + Nb) * F * H * W // 8 + 512
    assert_equal_counts(tuple(t.cpu().numpy() for t in got), torch_counts(a, b, size))        # 3 600 words a mask


# ---- graphs and the compiler -------------------------------------------------------------------------------------------

def test_hip_graph_replay_with_changed_inputs_gives_the_changed_counts():
    import devis_amd
    size = (45, 96)
    a, b = O.blob_logits(5, 2, 12, 20, 351).float().to(DEV), O.blob_logits(4, 2, 12, 20, 352).float().to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        devis_amd.mask_binary_iou(a, b, size)         # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        inter, area_a, area_b = devis_amd.mask_binary_iou_terms(a, b, size)
        iou = devis_amd.mask_binary_iou(a, b, size, reduce="frame")
    a2 = O.blob_logits(5, 2, 12, 20, 353).float().to(DEV)
    before = inter.clone()
    a.copy_(a2)
    for _ in range(2):          # (a replay adds onto nothing: the call zeroes its outputs itself)
        graph.replay()
    torch.cuda.synchronize()
    want = devis_amd.mask_binary_iou_terms(a2, b, size)
    assert torch.equal(inter, want[0]) and torch.equal(area_a, want[1]) and torch.equal(area_b, want[2])
    assert not torch.equal(inter, before)
    assert_equal_counts(tuple(t.cpu().numpy() for t in want), torch_counts(a2, b, size))
    assert torch.equal(iou, devis_amd.mask_binary_iou(a2, b, size, reduce="frame"))


def test_compile_fullgraph_equals_eager_also_with_dynamic_shapes():
    import devis_amd

    def fn(u, v, H, W):
        return devis_amd.mask_binary_iou_terms(u, v, (H, W)) + (devis_amd.mask_binary_iou(u, v, (H, W), reduce="frame"),)

    compiled = torch.compile(fn, fullgraph=True, dynamic=True)
    for n, (H, W) in ((3, (27, 35)), (5, (27, 35)), (4, (31, 20))):
        u = O.blob_logits(n, 2, 7, 9, 360 + n).float().to(DEV)
        v = O.blob_logits(n + 1, 2, 7, 9, 370 + n).float().to(DEV)
        got, want = compiled(u, v, H, W), fn(u, v, H, W)
        assert all(torch.equal(x, y) for x, y in zip(got, want))
        assert tuple(got[0].shape) == (n, n + 1, 2) and tuple(got[3].shape) == (n, n + 1) and got[3].dtype == F64
    static = torch.compile(lambda u, v: devis_amd.mask_binary_iou(u, v, (27, 35)), fullgraph=True)
    assert torch.equal(static(u, v), devis_amd.mask_binary_iou(u, v, (27, 35)))


# ---- integration -----------------------------------------------------------------------------------------------------

def _stitch_two_clips(tm, mm, tracker, clip_a, clip_b, size):
    """Two clips of 5 frames with overlap 2 through the patched stand-ins: (video tracks, clip tracks, the two costs)."""
    video = [tm.Track(i, tracker.process_masks(0, 0, size, clip_a[i]), last_t=5) for i in range(clip_a.shape[0])]
    clip = [tm.Track(j, tracker.process_masks(0, 1, size, clip_b[j])) for j in range(clip_b.shape[0])]
    matcher = tracker.hungarian_matcher
    return video, clip, (matcher.compute_volumetric_iou_cost(video, clip), matcher.compute_frame_average_iou_cost(video, clip))


@pytest.mark.parametrize("gpu_rle", [False, True])
def test_patched_tracker_in_binary_mode_end_to_end(gpu_rle):
    import devis_amd
    from test_maskbiou_cpu import binary_modules
    tm, mm, tracker = binary_modules(overlap=2)
    if gpu_rle:
        tm.mask_util.frPyObjects = lambda obj, h, w: {"size": [h, w], "counts": b"packed"}
    previous = devis_amd.patch_tracker(tm, mm, gpu_binary_iou=True, gpu_rle=gpu_rle)
    try:
        size = (45, 80)
        clip_a, clip_b = O.blob_logits(4, 5, 12, 20, 101).float().to(DEV), O.blob_logits(3, 5, 12, 20, 102).float().to(DEV)
        video, clip, (volume, frame) = _stitch_two_clips(tm, mm, tracker, clip_a, clip_b, size)
        assert [isinstance(m, dict) for m in video[0].masks] == [True, True, True, False, False]
        assert [isinstance(m, dict) for m in clip[0].masks] == [False, False, True, False, False]
        bits_a, bits_b = binarized(clip_a[:, 3:], size), binarized(clip_b[:, :2], size)
        for cost, reference in ((volume, B.reference_volume), (frame, B.reference_frame)):
            assert cost.dtype == np.float64 and cost.shape == (4, 3)
            assert np.array_equal(cost, reference(list(bits_a), list(bits_b)))
        assert volume.max() > 0.3
        # a frame without a detection
        video[2].masks[4] = None
        windows = [list(w) for w in bits_a]
        windows[2][1] = None
        assert np.array_equal(tracker.hungarian_matcher.compute_volumetric_iou_cost(video, clip), B.reference_volume(windows, list(bits_b)))
        # the trailing window is encoded on the way out
        for track in video + clip:
            result = track.get_formatted_result(3)
            assert all(m is None or isinstance(m, dict) for m in result["segmentations"])
            assert all(m is None or (isinstance(m["counts"], str) and m["size"] == list(size)) for m in result["segmentations"])
        assert video[2].get_formatted_result(3)["segmentations"][4] is None
    finally:
        devis_amd.unpatch_tracker(tm, mm, previous)


def test_the_patched_route_gives_the_unpatched_routes_dicts_with_the_real_encoder():
    """What rests on pycocotools' published source, checked with the package itself where it can be imported (elsewhere this
    test says that it was not): that the final segmentations equal those of binary mode without the keyword; that
    ``mask_util.iou`` gives 0.0, not NaN, for two masks without a set pixel -- the empty-pair convention of ``"frame"``; and
    that both reduces equal the reference's own arithmetic on real encodings (``mask_util.iou`` per frame and the mean;
    ``merge`` / ``area`` per pair).  Both sides are the correctly rounded float64 quotient of the same two integers, so the
    comparison is ``==``."""
    mask_util = pytest.importorskip("pycocotools.mask", reason="pycocotools is not installed: that the final dicts of "
                                    "gpu_binary_iou=True equal those of the unpatched binary mode, and that mask_util.iou "
                                    "gives 0 for an empty pair, was not checked here")
    import devis_amd
    from test_maskbiou_cpu import binary_modules
    size = (45, 80)
    clip_a, clip_b = O.blob_logits(4, 5, 12, 20, 101).float().to(DEV), O.blob_logits(3, 5, 12, 20, 102).float().to(DEV)
    results = []
    for kw in (dict(gpu_binary_iou=True), dict()):
        tm, mm, tracker = binary_modules(overlap=2)
        tm.mask_util = mask_util
        previous = devis_amd.patch_tracker(tm, mm, **kw)
        try:
            video = [tm.Track(i, tracker.process_masks(0, 0, size, clip_a[i]), last_t=5) for i in range(4)]
            clip = [tm.Track(j, tracker.process_masks(0, 1, size, clip_b[j])) for j in range(3)]
            results.append([t.get_formatted_result(1)["segmentations"] for t in video + clip])
        finally:
            devis_amd.unpatch_tracker(tm, mm, previous)
    assert results[0] == results[1]

    encode = lambda bits: mask_util.encode(np.asfortranarray(bits.astype(np.uint8)))      # noqa: E731
    # the stitching windows of the end-to-end case, with an empty frame and a track without a set pixel among them
    a, b = clip_a[:, 3:].clone(), clip_b[:, :2].clone()
    a[1, 1], b[2] = -1.0, -3.0
    bits_a, bits_b = binarized(a, size), binarized(b, size)
    assert not bits_a[1, 1].any() and not bits_b[2].any() and bits_a[0].any()
    rle_a, rle_b = [[encode(m) for m in w] for w in bits_a], [[encode(m) for m in w] for w in bits_b]
    # compute_frame_average_iou_cost with compute_iou_matrix: mask_util.iou per frame, stacked, the mean over the frames
    per_frame = [np.asarray(mask_util.iou([w[t] for w in rle_a], [w[t] for w in rle_b], [False] * len(rle_b))) for t in range(2)]
    frame = np.stack(per_frame, axis=0).mean(axis=0)
    got = devis_amd.mask_binary_iou(a, b, size, reduce="frame").cpu().numpy()
    want = B.reference_frame(list(bits_a), list(bits_b))
    # first the pairs that have a set pixel in every frame, then all of them: the only pair with a frame in which neither
    # mask has a pixel is (1, 2), whose ratio there the operator and the oracle take as 0.0
    both_empty = np.array([[any(not d.any() and not g.any() for d, g in zip(wa, wb)) for wb in bits_b] for wa in bits_a])
    assert both_empty.sum() == 1 and both_empty[1, 2] and frame.shape == (4, 3) and frame[~both_empty].max() > 0.2
    assert np.array_equal(got[~both_empty], frame[~both_empty]) and np.array_equal(want[~both_empty], frame[~both_empty])
    assert (got[:, 2] == 0.0).all() and (want[:, 2] == 0.0).all()
    # HungarianInferenceMatcher.iou: merge and area twice per pair and frame
    volume = np.zeros((4, 3))
    for i, j in np.ndindex(volume.shape):
        inter = sum(float(mask_util.area(mask_util.merge([d, g], True))) for d, g in zip(rle_a[i], rle_b[j]))
        union = sum(float(mask_util.area(mask_util.merge([d, g], False))) for d, g in zip(rle_a[i], rle_b[j]))
        volume[i, j] = inter / union if union > .0 else .0
    assert np.array_equal(devis_amd.mask_binary_iou(a, b, size, reduce="volume").cpu().numpy(), volume)
    assert np.array_equal(B.reference_volume(list(bits_a), list(bits_b)), volume)
    # the empty pair: 0.0, not NaN, from the package too
    none, some = encode(np.zeros(size, bool)), encode(np.ones(size, bool))
    assert np.asarray(mask_util.iou([none], [some], [False])).tolist() == [[0.0]]
    assert np.asarray(mask_util.iou([none], [none], [False])).tolist() == [[0.0]]
    assert np.array_equal(got, frame) and np.array_equal(want, frame)
