"""Times devis_amd.mask_losses against the PyTorch formulation of the reference's SetCriterion.loss_masks on the same GPU, in
the same process and dtype:

    t = target.to(src); x = F.interpolate(src[:, None], size, mode="bilinear", align_corners=False)[:, 0].flatten(1)
    sigmoid_focal_loss(x, t, num_boxes) and dice_loss(x, t, num_boxes)      (written out with torch's operators)

Shapes: N in {6, 36, 120} instances (trajectories x frames); logits at 1/4 and 1/8 of padded targets of 360x640 and 800x1333;
f32 and bf16 logits; forward and forward + backward.  The operator reads the bool target; the baseline converts it to a float
tensor as the reference does, inside the timed region.

    python scripts/maskloss_bench.py [--out profiles/maskloss_bench.json] [--windows 5] [--iters 10]

Device events after warm-up; operator and baseline windows alternate; the median of the windows is quoted and every window is
kept.  "overlap" is true when the fastest baseline window is not slower than the slowest operator window.  "bytes_fraction" is
the operator's algorithmic bytes (N*P target bytes once in the forward and once in the backward, the logits and their
gradient) over its time, as a fraction of 8 TB/s.
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

INSTANCES = (6, 36, 120)
TARGETS = ((360, 640), (800, 1333))
STRIDES = (4, 8)
HBM_BYTES_PER_S = 8e12


def baseline(src, target, num_boxes, alpha=0.25, gamma=2.0):
    t = target.to(src)
    x = F.interpolate(src[:, None], size=target.shape[-2:], mode="bilinear", align_corners=False)[:, 0].flatten(1)
    t = t.flatten(1)
    p = x.sigmoid()
    loss = F.binary_cross_entropy_with_logits(x, t, reduction="none") * ((1 - (p * t + (1 - p) * (1 - t))) ** gamma)
    loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    q = x.sigmoid()
    dice = 1 - (2 * (q * t).sum(1) + 1) / (q.sum(-1) + t.sum(-1) + 1)
    return loss.mean(1).sum() / num_boxes + dice.sum() / num_boxes


def fused(src, target, num_boxes):
    import devis_amd
    out = devis_amd.mask_losses(src, target, num_boxes)
    return out["loss_mask"] + out["loss_dice"]


def window(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maskloss_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--max-pixels", type=float, default=float("inf"), help="skip rows with more than this many N*H*W")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("maskloss_bench: no GPU; nothing is measured on the CPU")
    dev = torch.device("cuda:0")
    rows = []
    for dtype in (torch.float32, torch.bfloat16):
        for H, W in TARGETS:
            for stride in STRIDES:
                h, w = -(-H // stride), -(-W // stride)
                for N in INSTANCES:
                    if N * H * W > args.max_pixels:
                        continue
                    g = torch.Generator().manual_seed(N + H)
                    src = (2.5 * torch.randn(N, h, w, generator=g)).to(dev, dtype).requires_grad_(True)
                    target = (torch.rand(N, H // 8, W // 8, generator=g) > 0.6).to(dev)
                    target = F.interpolate(target[:, None].float(), size=(H, W), mode="nearest")[:, 0] > 0.5
                    num_boxes = float(N)
                    for backward in (False, True):
                        def run(fn):
                            loss = fn(src, target, num_boxes)
                            if backward:
                                torch.autograd.grad(loss, src)
                        calls = {"fused": lambda: run(fused), "pytorch": lambda: run(baseline)}
                        for fn in calls.values():       # warm-up: code objects, the allocator
                            for _ in range(3):
                                fn()
                        torch.cuda.synchronize()
                        times = {k: [] for k in calls}
                        for _ in range(args.windows):
                            for k, fn in calls.items():
                                times[k].append(window(fn, args.iters))
                        med = {k: statistics.median(v) for k, v in times.items()}
                        es = torch.empty((), dtype=dtype).element_size()
                        nbytes = N * H * W * (2 if backward else 1) + N * h * w * es * (3 if backward else 1)
                        row = {"dtype": str(dtype).replace("torch.", ""), "N": N, "src": [h, w], "target": [H, W],
                               "pass": "forward+backward" if backward else "forward",
                               "fused_ms": med["fused"], "pytorch_ms": med["pytorch"], "speedup": med["pytorch"] / med["fused"],
                               "fused_windows_ms": times["fused"], "pytorch_windows_ms": times["pytorch"],
                               "overlap": min(times["pytorch"]) <= max(times["fused"]),
                               "bytes_fraction": nbytes / (med["fused"] * 1e-3) / HBM_BYTES_PER_S}
                        rows.append(row)
                        print("%-8s N=%-3d %4dx%-4d -> %4dx%-4d %-16s fused %8.3f ms  pytorch %8.3f ms  x%.1f%s"
                              % (row["dtype"], N, h, w, H, W, row["pass"], med["fused"], med["pytorch"], row["speedup"],
                                 "  OVERLAP" if row["overlap"] else ""), flush=True)
                    del src, target
                    torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows, "iters": args.iters,
           "method": "device events around `iters` calls; windows of the two sides alternate; medians quoted", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
