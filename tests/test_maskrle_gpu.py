"""GPU tests of the run-length encoder (include/maskrle.h): the rows against ``binarize_masks`` at every pixel and against the
independent oracle, exact bit patterns at the edges of the packed words and of the bits pass's tiles, larger maps, the cap,
independence of batch, workspace and run, special values, memory, HIP graphs and torch.compile, and the stand-in tracker patched
with ``gpu_rle=True``.  Everything is integers: every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

import maskiou_oracle as O
import maskrle_oracle as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16]
F64 = torch.float64


def arith_of(dtype):
    return F64 if dtype == F64 else torch.float32


def tiles():
    from devis_amd import _maskrle as M
    return {k: M.tile(getattr(M, "TILE_" + k)) for k in ("BITS_PIXELS", "WORD_PIXELS", "BITS_SRC", "RUNS_THREADS")}


def default_cap(H, W):
    return min(H * W + 1, 8 * W + 1)


def expected_rows(bits, max_runs):
    """bits [N, H, W] numpy bool -> the rows include/maskrle.h promises, by the oracle."""
    rows = np.zeros((bits.shape[0], 1 + max_runs), dtype=np.int32)
    for n in range(bits.shape[0]):
        counts = R.runs_of(bits[n])
        rows[n, 0] = len(counts)
        keep = counts[:max_runs]
        rows[n, 1:1 + len(keep)] = keep
    return rows


def binarized(src, size):
    import devis_amd
    return devis_amd.binarize_masks(src, size, order="F").cpu().numpy()


def run_lengths(src, size, max_runs=None):
    import devis_amd
    rows = devis_amd.mask_run_lengths(src, size, max_runs=max_runs)
    cap = default_cap(*size) if max_runs is None else max_runs
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (src.shape[0], 1 + cap) and rows.is_contiguous()
    assert not rows.requires_grad and rows.device == src.device
    return rows.cpu().numpy()


# ---- binarise and the oracle ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("index", range(len(O.BINARIZE_CASES)))
def test_rows_decode_to_binarize_masks_at_every_pixel_and_to_the_oracle_outside_near_zero(index, dtype):
    src, size = O.binarize_case(index, dtype)
    H, W = size
    P = H * W
    rows = run_lengths(src.to(DEV), size, max_runs=P + 1)
    bits = binarized(src.to(DEV), size)
    want, x = O.binarize(src, size, arith_of(dtype))
    out = O.near_zero(x, src)
    assert float(out.double().mean()) <= O.BINARIZE_CAP
    for n in range(src.shape[0]):
        count = int(rows[n, 0])
        counts = rows[n, 1:1 + count]
        assert 1 <= count <= P + 1 and int(counts.sum()) == P and not rows[n, 1 + count:].any()
        decoded = R.decode(counts, H, W)
        assert np.array_equal(decoded, bits[n])                         # every pixel, without exception
        assert count == len(R.runs_of(bits[n])) and counts.tolist() == R.runs_of(bits[n])
        keep = ~out[n].numpy()
        assert np.array_equal(decoded[keep], want[n].numpy()[keep])     # the independent oracle
    print("runs %s of at most %d, default cap %d" % (rows[:, 0].tolist(), P + 1, default_cap(H, W)))
    if index == 4:
        assert src.shape[1] * src.shape[2] > tiles()["BITS_SRC"]         # not staged: the taps read memory
    # the default cap: the same rows, shorter, where it holds (pure noise at 45 x 80 stays under it)
    short = run_lengths(src.to(DEV), size)
    cap = default_cap(H, W)
    assert np.array_equal(short, expected_rows(bits, cap))
    assert int(rows[:, 0].max()) <= cap             # (on the CPU: 517 runs against 641 at 45 x 80, 76 against 89 at 13 x 11)
    if index == 0:
        assert cap == 641


# ---- exact bit patterns ----------------------------------------------------------------------------------------------

def _pattern_sizes():
    S = 4096        # (asserted against maskrle_tile in the test)
    return [(63, 65, S - 1), (8, 512, S), (17, 241, S + 1), (3, 2731, 2 * S + 1), (67, 61, None), (67, 62, None), (67, 123, None),
            (1, 130, None), (130, 1, None), (1, 1, None), (1, 64, None), (5, 13, None)]


def _patterns(P, S):
    """(name, walk [P] bool): masks given by their column-major walk."""
    q = np.arange(P)
    out = [("zeros", q < 0), ("ones", q >= 0)]
    for pos in (0, 1, 62, 63, 64, 65, S - 1, S, S + 1, 2 * S - 1, 2 * S, P - 2, P - 1):
        if 0 <= pos < P:
            out.append(("pixel %d" % pos, q == pos))
            out.append(("all but pixel %d" % pos, q != pos))
    for a, b in ((10, 64), (64, 100), (10, 63), (63, 65), (0, 64), (64, 128), (S - 5, S), (S, S + 7), (S - 5, S + 7), (60, S), (64, P),
                 (0, P - 1), (1, P), (S - 64, S + 64), (2 * S - 1, 2 * S + 1)):
        if 0 <= a < b <= P:
            out.append(("run %d:%d" % (a, b), (q >= a) & (q < b)))
    out += [("alternating from 1", q % 2 == 0), ("alternating from 0", q % 2 == 1),
            ("alternating words from 1", (q // 64) % 2 == 0), ("alternating words from 0", (q // 64) % 2 == 1),
            ("alternating lanes", (q // 16) % 2 == 0), ("alternating tiles", (q // S) % 2 == 1)]
    return out


@pytest.mark.parametrize("H,W,P_is", _pattern_sizes())
def test_exact_bit_patterns_through_an_identity_resample(H, W, P_is):
    S = tiles()["BITS_PIXELS"]
    assert S == 4096 and tiles()["WORD_PIXELS"] == 64
    P = H * W
    assert P_is is None or P == P_is
    names, walks = zip(*_patterns(P, S))
    bits = np.stack([wk.reshape(W, H).T for wk in walks])             # [N, H, W]
    src = torch.from_numpy(np.where(bits, 1.0, -1.0).astype(np.float32)).to(DEV)
    assert np.array_equal(binarized(src, (H, W)), bits)               # the bits are chosen, not computed
    rows = run_lengths(src, (H, W), max_runs=P + 1)
    want = expected_rows(bits, P + 1)
    for n, name in enumerate(names):
        assert np.array_equal(rows[n], want[n]), (name, rows[n, :8], want[n, :8])
    by_name = dict(zip(names, rows))
    assert by_name["zeros"][:2].tolist() == [1, P] and by_name["ones"][:3].tolist() == [2, 0, P]
    assert by_name["alternating from 1"][0] == P + 1 and by_name["alternating from 0"][0] == P      # the most runs there are
    # the same in the other storage types (+1 and -1 are exact in each)
    for dtype in (F64, torch.bfloat16, torch.float16):
        assert np.array_equal(run_lengths(src.to(dtype), (H, W), max_runs=P + 1), want)


# ---- larger maps -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def large_case(kind):
    if kind == "blob":
        return O.blob_logits(3, 1, 12, 20, 201)[:, 0].float(), (90, 160)
    g = torch.Generator().manual_seed(202)
    return 2.5 * torch.randn(3, 12, 20, generator=g), (135, 240)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["blob", "noise"])
def test_larger_maps_over_several_workgroups_and_words_per_thread(kind, dtype):
    src, size = large_case(kind)
    src = src.to(dtype).to(DEV)
    P = size[0] * size[1]
    assert P > 3 * tiles()["BITS_PIXELS"]
    if kind == "noise":
        assert P > tiles()["RUNS_THREADS"] * tiles()["WORD_PIXELS"]          # more than one word per thread of the runs pass
    bits = binarized(src, size)
    assert 0.02 < bits.mean() < 0.98
    rows = run_lengths(src, size, max_runs=P + 1)
    assert np.array_equal(rows, expected_rows(bits, P + 1))
    cap = default_cap(*size)
    print("%s: runs %s, default cap %d" % (kind, rows[:, 0].tolist(), cap))
    assert np.array_equal(run_lengths(src, size), expected_rows(bits, cap))
    if kind == "blob":
        assert int(rows[:, 0].max()) <= 2 * size[1] + 1 <= cap          # compact regions: two transitions per column


# ---- the cap ---------------------------------------------------------------------------------------------------------

def test_a_row_over_the_cap_keeps_its_true_count_and_the_prefix_and_nothing_is_written_outside():
    from devis_amd import _maskrle
    src, size = O.binarize_case(0)
    src = src.to(DEV)
    H, W = size
    bits = binarized(src, size)
    true = [len(R.runs_of(b)) for b in bits]
    assert min(true) > 100
    for max_runs in (1, 2, 63, min(true) - 1, min(true), max(true), max(true) + 1):
        rows = run_lengths(src, size, max_runs=max_runs)
        assert rows[:, 0].tolist() == true and np.array_equal(rows, expected_rows(bits, max_runs)), max_runs
    # the raw call into a sentinel-filled buffer, at an offset that is no multiple of 16 bytes
    max_runs = min(true) // 2
    n = 3 * (1 + max_runs)
    sentinel = 0x5a5a5a5a
    buf = torch.full((n + 64,), sentinel, dtype=torch.int32, device=DEV)
    out = buf[17:17 + n]
    assert out.data_ptr() % 16 != 0
    ws = torch.empty(_maskrle.workspace_bytes(3, H, W), dtype=torch.uint8, device=DEV)
    _maskrle.encode(0, src, 3, src.shape[1], src.shape[2], H, W, max_runs, ws, out)
    torch.cuda.synchronize()
    assert bool((buf[:17] == sentinel).all()) and bool((buf[17 + n:] == sentinel).all())
    got = out.view(3, 1 + max_runs).cpu().numpy()
    assert np.array_equal(got, expected_rows(bits, max_runs)) and (got[:, 0] > max_runs).all()


# ---- independence ----------------------------------------------------------------------------------------------------

def test_rows_do_not_depend_on_workspace_output_batch_run_or_strides():
    import devis_amd
    from devis_amd import _maskrle
    size = (67, 123)
    H, W = size
    src = O.blob_logits(7, 1, 9, 14, 211)[:, 0].float().to(DEV)
    cap = default_cap(H, W)
    first = devis_amd.mask_run_lengths(src, size)
    assert torch.equal(first, devis_amd.mask_run_lengths(src, size))                    # run to run
    want = expected_rows(binarized(src, size), cap)
    assert np.array_equal(first.cpu().numpy(), want)
    # stale memory: workspace and output full of 0x7f bytes
    ws = torch.full((_maskrle.workspace_bytes(7, H, W) + 64,), 0x7f, dtype=torch.uint8, device=DEV)
    out = torch.full((7, 1 + cap), 0x7f7f7f7f, dtype=torch.int32, device=DEV)
    _maskrle.encode(0, src, 7, 9, 14, H, W, cap, ws, out)
    torch.cuda.synchronize()
    assert torch.equal(out, first) and bool((ws[-64:] == 0x7f).all())
    # a mask alone, and a slice of the batch
    for n in range(7):
        assert torch.equal(devis_amd.mask_run_lengths(src[n:n + 1], size), first[n:n + 1]), n
    assert torch.equal(devis_amd.mask_run_lengths(src[2:5], size), first[2:5])
    # a view that is not dense, and logits at an address that is no multiple of 16 bytes
    wide = torch.stack([src, -src], 3).flatten(2)          # [7, 9, 28]: src in the even columns
    view = wide[:, :, ::2]
    assert not view.is_contiguous() and torch.equal(view, src)
    assert torch.equal(devis_amd.mask_run_lengths(view, size), first)
    base = torch.empty(src.numel() + 1, dtype=src.dtype, device=DEV)
    odd = base[1:].view(src.shape).copy_(src)
    assert odd.data_ptr() % 16 != 0
    assert torch.equal(devis_amd.mask_run_lengths(odd, size), first)
    # no maps
    empty = devis_amd.mask_run_lengths(src[:0], size)
    assert tuple(empty.shape) == (0, 1 + cap) and empty.dtype == torch.int32
    assert tuple(devis_amd.mask_run_lengths(src[:0], size, max_runs=5).shape) == (0, 6)


# ---- special values --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_logits(dtype):
    inf, nan = float("inf"), float("nan")
    size, P = (11, 19), 11 * 19
    maps = torch.zeros(7, 4, 5)
    maps[0], maps[1], maps[2], maps[3] = inf, -inf, nan, 100.0
    maps[4] = O.blob_logits(1, 1, 4, 5, 71)[0, 0].float()
    maps[5] = maps[4]
    maps[5, :2, :2] = inf                   # an infinite blob on a finite map
    maps[6] = maps[4]
    maps[6, 2, 2] = nan                     # a NaN logit: 0 bits wherever one of its taps has a nonzero weight
    src = maps.to(dtype).to(DEV)
    bits = binarized(src, size)
    rows = run_lengths(src, size, max_runs=P + 1)
    assert np.array_equal(rows, expected_rows(bits, P + 1))
    assert rows[0, :3].tolist() == [2, 0, P] and rows[3, :3].tolist() == [2, 0, P]
    assert rows[1, :2].tolist() == [1, P] and rows[2, :2].tolist() == [1, P]             # NaN everywhere: no bit set
    mark = torch.zeros(1, 4, 5, dtype=F64)
    mark[0, 2, 2] = 1.0
    hit = (O.logits(mark, size, arith_of(dtype))[0] > 0).numpy()
    decoded = R.decode(rows[6, 1:1 + rows[6, 0]], *size)
    assert hit.sum() >= 4 and not decoded[hit].any()
    assert np.array_equal(decoded[~hit], bits[4][~hit]) and bits[5].sum() >= bits[4].sum()


# ---- memory ----------------------------------------------------------------------------------------------------------

def test_peak_allocation_is_output_and_workspace_and_less_than_the_byte_map():
    import devis_amd
    from devis_amd import _maskrle
    N, size = 8, (720, 1280)
    H, W = size
    src = O.blob_logits(N, 1, 180, 320, 221)[:, 0].float().to(DEV)
    devis_amd.mask_run_lengths(src[:1], (45, 80))           # the library is loaded, the kernels are resident
    up = lambda n: (n + 511) // 512 * 512      # noqa: E731  (the caching allocator's granule)
    cap = default_cap(H, W)
    output, workspace = up(4 * N * (1 + cap)), up(_maskrle.workspace_bytes(N, H, W))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    rows = devis_amd.mask_run_lengths(src, size)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak %d, output %d, workspace %d, byte map %d" % (peak, output, workspace, N * H * W))
    assert peak <= output + workspace < N * H * W
    assert workspace <= N * H * W // 8 + 512
    # and the rows are right at this size: 14 400 words a mask, 57 a thread
    bits = binarized(src, size)
    assert np.array_equal(rows.cpu().numpy(), expected_rows(bits, cap))
    print("runs %s, default cap %d" % (rows[:, 0].tolist(), cap))


# ---- graphs and the compiler -------------------------------------------------------------------------------------------

def test_hip_graph_replay_with_changed_inputs_gives_the_changed_rows():
    import devis_amd
    size = (45, 96)
    a = O.blob_logits(5, 1, 12, 20, 231)[:, 0].float().to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        devis_amd.mask_run_lengths(a, size)         # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rows = devis_amd.mask_run_lengths(a, size)
    a2 = O.blob_logits(5, 1, 12, 20, 232)[:, 0].float().to(DEV)
    before = rows.clone()
    a.copy_(a2)
    graph.replay()
    torch.cuda.synchronize()
    want = devis_amd.mask_run_lengths(a2, size)
    assert torch.equal(rows, want) and not torch.equal(rows, before)
    assert np.array_equal(rows.cpu().numpy(), expected_rows(binarized(a2, size), default_cap(*size)))


def test_compile_fullgraph_equals_eager_also_with_dynamic_shapes():
    import devis_amd

    def fn(u, H, W):
        return devis_amd.mask_run_lengths(u, (H, W)), devis_amd.mask_run_lengths(u, (H, W), max_runs=40)

    compiled = torch.compile(fn, fullgraph=True, dynamic=True)
    for n, (H, W) in ((3, (27, 35)), (5, (27, 35)), (4, (31, 20))):
        u = O.blob_logits(n, 1, 7, 9, 240 + n)[:, 0].float().to(DEV)
        got, want = compiled(u, H, W), fn(u, H, W)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert tuple(got[0].shape) == (n, 1 + default_cap(H, W)) and tuple(got[1].shape) == (n, 41)


# ---- integration -----------------------------------------------------------------------------------------------------

def test_patched_tracker_with_gpu_rle_end_to_end():
    import devis_amd
    from test_maskiou_cpu import StandInTrack, stock_soft_iou
    from test_maskrle_cpu import rle_modules
    tm, mm, tracker = rle_modules(overlap=2)
    previous = devis_amd.patch_tracker(tm, mm, gpu_rle=True)
    try:
        size = (45, 80)
        clip_a, clip_b = O.blob_logits(4, 5, 12, 20, 101).float().to(DEV), O.blob_logits(3, 5, 12, 20, 102).float().to(DEV)
        video = [StandInTrack(i, tracker.process_masks(0, 0, size, clip_a[i]), last_t=5) for i in range(4)]
        clip = [StandInTrack(j, tracker.process_masks(0, 1, size, clip_b[j])) for j in range(3)]
        assert [isinstance(m, dict) for m in video[0].masks] == [True, True, True, False, False]
        assert [isinstance(m, dict) for m in clip[0].masks] == [False, False, True, False, False]
        for track in video + clip:
            for m in track.masks:
                assert isinstance(m, devis_amd.LogitMask) or (isinstance(m["counts"], str) and m["size"] == list(size))
        packed = tm.mask_util.packed
        assert len(packed) == 4 * 3 + 3 * 1 and tm.mask_util.seen == []          # one pack per encoded frame, no encode
        k = 0
        for maps, frames in [(clip_a[i], (0, 1, 2)) for i in range(4)] + [(clip_b[j], (2,)) for j in range(3)]:
            bits = binarized(maps, size)
            for t in frames:
                obj, h, w = packed[k]
                k += 1
                assert (h, w) == size and obj["size"] == list(size) and all(type(c) is int for c in obj["counts"])
                assert np.array_equal(R.decode(obj["counts"], *size), bits[t])
        matcher = tracker.hungarian_matcher
        for fn, reduce in ((matcher.compute_volumetric_iou_cost, "volume"), (matcher.compute_frame_average_iou_cost, "frame")):
            cost = fn(video, clip)
            want = stock_soft_iou(clip_a[:, 3:].double().cpu(), clip_b[:, :2].double().cpu(), size, reduce)
            assert cost.shape == (4, 3) and float(np.abs(cost - want.numpy()).max()) <= 1e-4 * float(want.abs().max())
        rle = tm.encode_mask(video[0].masks[3])
        assert rle["size"] == list(size) and isinstance(rle["counts"], str) and len(packed) == 16 and tm.mask_util.seen == []
    finally:
        devis_amd.unpatch_tracker(tm, mm, previous)


def test_both_routes_give_equal_dicts_with_the_real_encoder():
    """That ``frPyObjects`` on the counts equals ``encode`` on the bytes rests on pycocotools' published source; where the
    package is installed it is checked on real masks, elsewhere this test says that it was not."""
    mask_util = pytest.importorskip("pycocotools.mask", reason="pycocotools is not installed: that frPyObjects on the counts "
                                    "equals encode on the byte map was not checked here")
    from devis_amd import tracking
    size = (45, 80)
    g = torch.Generator().manual_seed(250)
    maps = torch.cat([O.blob_logits(4, 1, 12, 20, 101)[:, 0].float(), 2.5 * torch.randn(2, 12, 20, generator=g)]).to(DEV)
    want = tracking.encode_logits(maps, size, mask_util)
    assert tracking.encode_logits_rle(maps, size, mask_util) == want
    assert tracking.encode_logits_rle(maps, size, mask_util, max_runs=200) == want          # some through the byte path
