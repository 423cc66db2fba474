"""Times the binary mask IoU against three other ways to the same cost matrix, on the same GPU, in the same process and dtype.

devis_amd.mask_binary_iou(a, b, size) -- logits in, float64 [Na, Nb] out -- against:

    torch       devis_amd.binarize_masks on both operands, then one float32 batched matrix product of the flattened 0/1 maps
                (a count is below 2^24, so the product is exact), the areas as sums, the ratio: what a careful torch user
                would write on top of the existing binarise kernel.
    soft        devis_amd.mask_soft_iou at the same shapes: the other stitching cost, which does strictly more per pixel.
    pair loop   the reference's HungarianInferenceMatcher.iou arithmetic -- mask_util.merge and mask_util.area twice per pair
                and frame -- on encodings that exist already, as in the reference.  Only where pycocotools is importable;
                elsewhere the rows say that it was not measured.

Shapes: Na = Nb in {10, 100} tracks, F = 2 overlap frames; logits at 1/4 and 1/8 of 360x640 and 720x1280; f32 and bf16.
Peak new allocations of each side are recorded beside the times.

    python scripts/maskbiou_bench.py [--out profiles/maskbiou_bench.json] [--windows 5] [--iters 10]

The method of scripts/maskiou_bench.py: device events after warm-up; the windows of the sides alternate; the median of the
windows is quoted and every window is kept.  The pair loop is host work and is timed over one call with a host clock.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TRACKS = (10, 100)
TARGETS = ((360, 640), (720, 1280))
STRIDES = (4, 8)
FRAMES = 2

try:
    from pycocotools import mask as mask_util
except ImportError:
    mask_util = None


def torch_formulation(devis_amd, a, b, size):
    Na, Nb, frames = a.shape[0], b.shape[0], a.shape[1]
    A = devis_amd.binarize_masks(a.flatten(0, 1), size).view(Na, frames, -1).transpose(0, 1).float()        # [F, Na, P]
    B = devis_amd.binarize_masks(b.flatten(0, 1), size).view(Nb, frames, -1).transpose(0, 1).float()
    inter = torch.bmm(A, B.transpose(1, 2)).sum(0).double()
    union = A.sum((0, 2)).double()[:, None] + B.sum((0, 2)).double()[None] - inter
    return inter / union.clamp(min=1.0)


def encodings(devis_amd, maps, size):
    """Per track the list of its frames' encodings, by mask_util.encode on the binarised maps."""
    bits = devis_amd.binarize_masks(maps.flatten(0, 1), size, order="F").transpose(1, 2).cpu().numpy()
    flat = [mask_util.encode(m.T) for m in bits]
    frames = maps.shape[1]
    return [flat[i * frames:(i + 1) * frames] for i in range(maps.shape[0])]


def pair_loop(tracks_a, tracks_b):
    """The reference's iou arithmetic over all pairs (every frame has a mask here)."""
    out = []
    for ma in tracks_a:
        row = []
        for mb in tracks_b:
            i, u = .0, .0
            for d, g in zip(ma, mb):
                i += mask_util.area(mask_util.merge([d, g], True))
                u += mask_util.area(mask_util.merge([d, g], False))
            row.append(i / u if u > .0 else .0)
        out.append(row)
    return out


def window(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maskbiou_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("maskbiou_bench: no GPU; nothing is measured on the CPU")
    import devis_amd
    from maskiou_oracle import blob_logits
    dev = torch.device("cuda:0")
    rows = []
    for dtype in (torch.float32, torch.bfloat16):
        for H, W in TARGETS:
            for stride in STRIDES:
                h, w = -(-H // stride), -(-W // stride)
                size = (H, W)
                for N in TRACKS:
                    a = F.interpolate(blob_logits(N, FRAMES, 12, 20, N + H).float(), size=(h, w), mode="bilinear").to(dev, dtype)
                    b = F.interpolate(blob_logits(N, FRAMES, 12, 20, N + H + 1).float(), size=(h, w), mode="bilinear").to(dev, dtype)
                    calls = {"fused": lambda: devis_amd.mask_binary_iou(a, b, size),
                             "torch": lambda: torch_formulation(devis_amd, a, b, size),
                             "soft": lambda: devis_amd.mask_soft_iou(a, b, size)}
                    for fn in calls.values():
                        for _ in range(3):
                            fn()
                    torch.cuda.synchronize()
                    times = {k: [] for k in calls}
                    for _ in range(args.windows):
                        for k, fn in calls.items():
                            times[k].append(window(fn, args.iters))
                    med = {k: statistics.median(v) for k, v in times.items()}
                    peaks = {k: peak_of(fn) for k, fn in calls.items()}
                    fused = calls["fused"]()
                    row = {"dtype": str(dtype).replace("torch.", ""), "tracks": N, "frames": FRAMES, "src": [h, w], "target": [H, W],
                           "fused_ms": med["fused"], "torch_ms": med["torch"], "soft_ms": med["soft"],
                           "torch_over_fused": med["torch"] / med["fused"], "soft_over_fused": med["soft"] / med["fused"],
                           "fused_windows_ms": times["fused"], "torch_windows_ms": times["torch"], "soft_windows_ms": times["soft"],
                           "overlap_torch": min(times["torch"]) <= max(times["fused"]),
                           "overlap_soft": min(times["soft"]) <= max(times["fused"]),
                           "fused_peak_bytes": peaks["fused"], "torch_peak_bytes": peaks["torch"], "soft_peak_bytes": peaks["soft"],
                           "equals_torch": bool(torch.equal(fused, calls["torch"]())),
                           "mean_iou": float(fused.mean()), "max_iou": float(fused.max())}
                    if mask_util is None:
                        row["pair_loop"] = "not measured: pycocotools is not importable here"
                    else:
                        tracks_a, tracks_b = encodings(devis_amd, a, size), encodings(devis_amd, b, size)
                        start = time.perf_counter()
                        host = pair_loop(tracks_a, tracks_b)
                        row["pair_loop_ms"] = (time.perf_counter() - start) * 1e3
                        row["pair_loop_over_fused"] = row["pair_loop_ms"] / med["fused"]
                        row["equals_pair_loop"] = bool(torch.equal(fused.cpu(), torch.tensor(host, dtype=torch.float64)))
                    rows.append(row)
                    print("%-8s N=%-3d %4dx%-4d -> %4dx%-4d fused %8.3f ms (%6.1f MB)  torch %8.3f ms (%7.1f MB)  soft %8.3f ms  "
                          "pair loop %s%s" % (row["dtype"], N, h, w, H, W, med["fused"], peaks["fused"] / 1e6, med["torch"],
                                              peaks["torch"] / 1e6, med["soft"],
                                              "%.1f ms" % row["pair_loop_ms"] if "pair_loop_ms" in row else "not measured",
                                              "" if row["equals_torch"] else "  DIFFERS"), flush=True)
                    del a, b
                    torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows, "iters": args.iters,
           "method": "device events around `iters` calls; windows of the sides alternate; medians quoted; the pair loop is one "
                     "call on encodings that exist already, by a host clock, where pycocotools is importable",
           "pycocotools": mask_util is not None, "binary_iou": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
