"""Times the run-length encoder against the byte path it replaces, on the same GPU, in the same process and dtype.

    (a) device   devis_amd.mask_run_lengths(src, size)  against  devis_amd.binarize_masks(src, size, order="F")
    (b) wall     operator + host copy of the rows       against  binarise + host copy of one byte per pixel
    (c) host     mask_util.frPyObjects on the counts    against  mask_util.encode on the byte map -- only where pycocotools
                 is importable; otherwise the rows say that it was not measured

Beside the times: the bytes each route copies to the host, and the largest number of runs of a mask against the default cap.

Shapes: N in {1, 10, 100} blob logit maps at 1/4 and 1/8 of 360x640 and 720x1280; f32 and bf16.

    python scripts/maskrle_bench.py [--out profiles/maskrle_bench.json] [--windows 5] [--iters 10]

(a): device events after warm-up; windows of the two sides alternate; the median of the windows is quoted and every window is
kept.  (b) and (c): time.perf_counter around the same number of calls, the device idle before and after each window.  A row
whose windows overlap is marked and is not a difference.
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

MAPS = (1, 10, 100)
TARGETS = ((360, 640), (720, 1280))
STRIDES = (4, 8)


def window(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def wall_window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def alternate(calls, timer, windows, iters):
    """{name: the windows' times in ms}, the sides taking turns."""
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(windows):
        for k, fn in calls.items():
            times[k].append(timer(fn, iters))
    return times


def compare(times, ours, theirs):
    med = {k: statistics.median(v) for k, v in times.items()}
    return {ours + "_ms": med[ours], theirs + "_ms": med[theirs], theirs + "_over_" + ours: med[theirs] / med[ours],
            ours + "_windows_ms": times[ours], theirs + "_windows_ms": times[theirs],
            "overlap": min(times[theirs]) <= max(times[ours]) and min(times[ours]) <= max(times[theirs])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maskrle_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("maskrle_bench: no GPU; nothing is measured on the CPU")
    import devis_amd
    from maskiou_oracle import blob_logits
    try:
        from pycocotools import mask as mask_util
    except ImportError:
        mask_util = None
    dev = torch.device("cuda:0")
    rows = []
    for dtype in (torch.float32, torch.bfloat16):
        for H, W in TARGETS:
            for stride in STRIDES:
                h, w = -(-H // stride), -(-W // stride)
                size = (H, W)
                for N in MAPS:
                    src = F.interpolate(blob_logits(N, 1, 12, 20, N + H).float(), size=(h, w), mode="bilinear")[:, 0].to(dev, dtype)
                    rle = lambda: devis_amd.mask_run_lengths(src, size)                      # noqa: E731
                    binarise = lambda: devis_amd.binarize_masks(src, size, order="F")        # noqa: E731
                    runs = rle()
                    cap = runs.shape[1] - 1
                    most = int(runs[:, 0].max())
                    row = {"dtype": str(dtype).replace("torch.", ""), "maps": N, "src": [h, w], "target": [H, W],
                           "max_runs_of_a_mask": most, "default_cap": cap,
                           "rle_bytes_copied": runs.numel() * runs.element_size(), "bytes_bytes_copied": N * H * W}
                    device = compare(alternate({"rle": rle, "binarize": binarise}, window, args.windows, args.iters), "rle", "binarize")
                    row["device"] = device
                    wall = compare(alternate({"rle": lambda: rle().cpu(), "binarize": lambda: binarise().transpose(1, 2).cpu()},
                                             wall_window, args.windows, args.iters), "rle", "binarize")
                    row["wall_with_host_copy"] = wall
                    if mask_util is None:
                        row["host_packing"] = "not measured: pycocotools is not importable here"
                    else:
                        host_runs = runs.cpu().numpy()
                        host_bits = binarise().transpose(1, 2).cpu().numpy()

                        def pack():
                            return [mask_util.frPyObjects({"size": [H, W], "counts": host_runs[n, 1:1 + host_runs[n, 0]].tolist()}, H, W)
                                    for n in range(N) if host_runs[n, 0] <= cap]

                        def encode():
                            return [mask_util.encode(host_bits[n].T) for n in range(N)]

                        same = all(p == e for p, e in zip(pack(), encode())) if most <= cap else None
                        row["host_packing"] = dict(compare(alternate({"frpyobjects": pack, "encode": encode}, wall_window,
                                                                     args.windows, 1), "frpyobjects", "encode"), equal_encodings=same)
                    rows.append(row)
                    print("%-8s N=%-3d %4dx%-4d -> %4dx%-4d device rle %7.3f ms, binarise %7.3f ms%s | with copy rle %8.3f ms (%9d B), "
                          "bytes %8.3f ms (%10d B)%s | runs %d of %d"
                          % (row["dtype"], N, h, w, H, W, device["rle_ms"], device["binarize_ms"], " OVERLAP" if device["overlap"] else "",
                             wall["rle_ms"], row["rle_bytes_copied"], wall["binarize_ms"], row["bytes_bytes_copied"],
                             " OVERLAP" if wall["overlap"] else "", most, cap), flush=True)
                    del src, runs
                    torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows, "iters": args.iters,
           "pycocotools": mask_util is not None,
           "method": "device: device events around `iters` calls; wall_with_host_copy and host_packing: perf_counter around the "
                     "calls with the device idle before and after; windows of the two sides alternate; medians quoted, every "
                     "window kept; rows marked overlap are not a difference", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
