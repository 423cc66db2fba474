"""Times the clip-stitching operators against PyTorch formulations on the same GPU, in the same process and dtype.

devis_amd.mask_soft_iou(a, b, size) -- logits in, [Na, Nb] out -- against two formulations:

    pair loop   the reference's HungarianInferenceMatcher.compute_volumetric_iou_cost: for every pair, soft_iou on the
                stacked full-resolution probability maps (three elementwise kernels, two reductions, an .item()).  The maps
                exist already, as in the reference (Tracker.process_masks made them); making them is not in this time.
    fair        upsample everything once, sigmoid, one pa @ pb.T, the sums, the ratio: what a careful torch user would write.
                Making the maps is in this time, as it is in the operator's.

devis_amd.binarize_masks(src, size, order="F") against F.interpolate(src).sigmoid() > 0.5.

Shapes: Na = Nb in {10, 50, 100} tracks, F = 2 overlap frames; logits at 1/4 and 1/8 of 360x640 and 720x1280; f32 and bf16.
Peak new allocations of each side are recorded beside the times.

    python scripts/maskiou_bench.py [--out profiles/maskiou_bench.json] [--windows 5] [--iters 10]

Device events after warm-up; operator and fair windows alternate; the median of the windows is quoted and every window is
kept.  The pair loop synchronises ten thousand times a call at 100 tracks, so it is timed over one call.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TRACKS = (10, 50, 100)
TARGETS = ((360, 640), (720, 1280))
STRIDES = (4, 8)
FRAMES = 2


def probabilities(x, size):
    return F.interpolate(x, size=size, mode="bilinear", align_corners=False).sigmoid()


def fair(a, b, size, eps=1e-6):
    pa, pb = probabilities(a, size).flatten(1), probabilities(b, size).flatten(1)
    inter = (pa @ pb.t()).float()
    union = pa.sum(1, dtype=torch.float32)[:, None] + pb.sum(1, dtype=torch.float32)[None] - inter
    return inter / union.clamp(min=eps)


def soft_iou(m1, m2):
    """The reference's soft_iou on two lists of probability maps."""
    m1, m2 = torch.stack(m1), torch.stack(m2)
    i = (m1 * m2).sum()
    u = (m1 + m2 - m1 * m2).sum().clamp(1e-6)
    return (i / u).item() if u > .0 else .0


def pair_loop(maps_a, maps_b):
    return [[soft_iou(ma, mb) for mb in maps_b] for ma in maps_a]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maskiou_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-pair-loop", action="store_true", help="skip the reference's pair loop (minutes at 100 tracks)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("maskiou_bench: no GPU; nothing is measured on the CPU")
    import devis_amd
    from maskiou_oracle import blob_logits
    dev = torch.device("cuda:0")
    rows, bin_rows = [], []
    for dtype in (torch.float32, torch.bfloat16):
        for H, W in TARGETS:
            for stride in STRIDES:
                h, w = -(-H // stride), -(-W // stride)
                size = (H, W)
                for N in TRACKS:
                    a = F.interpolate(blob_logits(N, FRAMES, 12, 20, N + H).float(), size=(h, w), mode="bilinear").to(dev, dtype)
                    b = F.interpolate(blob_logits(N, FRAMES, 12, 20, N + H + 1).float(), size=(h, w), mode="bilinear").to(dev, dtype)
                    calls = {"fused": lambda: devis_amd.mask_soft_iou(a, b, size), "fair": lambda: fair(a, b, size)}
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
                    err = float((calls["fused"]() - calls["fair"]()).abs().max())
                    row = {"dtype": str(dtype).replace("torch.", ""), "tracks": N, "frames": FRAMES, "src": [h, w], "target": [H, W],
                           "fused_ms": med["fused"], "fair_ms": med["fair"], "fair_over_fused": med["fair"] / med["fused"],
                           "fused_windows_ms": times["fused"], "fair_windows_ms": times["fair"],
                           "overlap": min(times["fair"]) <= max(times["fused"]),
                           "fused_peak_bytes": peaks["fused"], "fair_peak_bytes": peaks["fair"], "max_abs_difference": err}
                    if not args.no_pair_loop:
                        pa, pb = probabilities(a, size), probabilities(b, size)
                        maps_a, maps_b = [list(m) for m in pa], [list(m) for m in pb]
                        pair_loop(maps_a[:2], maps_b[:2])
                        row["pair_loop_ms"] = window(lambda: pair_loop(maps_a, maps_b), 1)
                        row["pair_loop_resident_bytes"] = (pa.numel() + pb.numel()) * pa.element_size()
                        row["pair_loop_over_fused"] = row["pair_loop_ms"] / med["fused"]
                        del pa, pb, maps_a, maps_b
                    rows.append(row)
                    print("%-8s N=%-3d %4dx%-4d -> %4dx%-4d fused %8.3f ms (%6.1f MB)  fair %8.3f ms (%7.1f MB)  pair loop %10.1f ms%s"
                          % (row["dtype"], N, h, w, H, W, med["fused"], peaks["fused"] / 1e6, med["fair"], peaks["fair"] / 1e6,
                             row.get("pair_loop_ms", float("nan")), "  OVERLAP" if row["overlap"] else ""), flush=True)
                    if N == TRACKS[-1]:
                        src = a[:, 0].contiguous()
                        calls = {"fused": lambda: devis_amd.binarize_masks(src, size, order="F"),
                                 "pytorch": lambda: probabilities(src[:, None], size)[:, 0] > 0.5}
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
                        differ = int((calls["fused"]() != calls["pytorch"]()).sum())
                        bin_rows.append({"dtype": row["dtype"], "maps": N, "src": [h, w], "target": [H, W], "fused_ms": med["fused"],
                                         "pytorch_ms": med["pytorch"], "pytorch_over_fused": med["pytorch"] / med["fused"],
                                         "fused_windows_ms": times["fused"], "pytorch_windows_ms": times["pytorch"],
                                         "overlap": min(times["pytorch"]) <= max(times["fused"]),
                                         "fused_peak_bytes": peaks["fused"], "pytorch_peak_bytes": peaks["pytorch"],
                                         "differing_pixels": differ})
                        print("%-8s binarise N=%-3d %4dx%-4d -> %4dx%-4d fused %8.3f ms (%6.1f MB)  pytorch %8.3f ms (%7.1f MB)"
                              % (row["dtype"], N, h, w, H, W, med["fused"], peaks["fused"] / 1e6, med["pytorch"],
                                 peaks["pytorch"] / 1e6), flush=True)
                    del a, b
                    torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows, "iters": args.iters,
           "method": "device events around `iters` calls; windows of the two sides alternate; medians quoted; the pair loop is "
                     "one call on probability maps that exist already", "soft_iou": rows, "binarize": bin_rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
