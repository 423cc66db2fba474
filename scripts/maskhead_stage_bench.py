"""Times devis_amd.mask_head_stage on the five stages of the mask head of a 360x640 clip (F = 6 frames): 264 @ 12x20 plain,
128 @ 12x20 -> 23x40 + 8 maps, 64 @ 23x40 -> 45x80 + 8, 32 @ 45x80 -> 90x160, 16 @ 90x160 plain; 10 and 50 trajectories
(N = 60, 300); f32, and bf16 with float32 parameters and maps; forward and forward + backward.  The baseline is the PyTorch
chain the reference runs between two convolutions, ending in the channels-last copy deform_conv2d makes of its input, on the
same GPU, in the same process and dtype:

    x = relu(group_norm(x)); cur = skip.repeat(n, 1, 1, 1); x = cur + interpolate(x, size, "nearest"); x = cat([x, maps], 1)
    x.permute(0, 2, 3, 1).contiguous()

    python scripts/maskhead_stage_bench.py [--out profiles/maskhead_stage_bench.json] [--windows 5] [--iters 20] [--no-module]

Device events after warm-up; operator and baseline windows alternate; the median of the windows is quoted and every window is
kept.  "hbm_fraction" is the operator's algorithmic bytes (x read twice, skip's F images and the maps
read once, out written once; backward: grad_out read twice -- for dy and for grad_skip --, x read twice, dy written and read,
grad_x and grad_skip written) over its time, as a fraction of 8 TB/s.  A last row times the whole MaskHeadConv, forward +
backward at N = 60, with the HIP convolutions on both sides: the module of this package against the same layers with the
PyTorch glue.
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

FRAMES, GROUPS = 6, 8
# (C, E, (h, w), (H, W), merge)
STAGES = [(264, 0, (12, 20), (12, 20), False), (128, 8, (12, 20), (23, 40), True), (64, 8, (23, 40), (45, 80), True),
          (32, 0, (45, 80), (90, 160), True), (16, 0, (90, 160), (90, 160), False)]
TRAJECTORIES = (10, 50)
HBM_BYTES_PER_S = 8e12


def make(stage, n_traj, dtype, dev):
    C, E, hw, HW, merge = stage
    N = FRAMES * n_traj
    gen = torch.Generator().manual_seed(C + N)
    rnd = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    t = {"x": (1.5 * rnd(N, C, *hw) + 0.3).to(dev, dtype), "weight": (0.5 * rnd(C) + 1).to(dev), "bias": (0.3 * rnd(C)).to(dev),
         "skip": rnd(FRAMES, C, *HW).to(dev, dtype) if merge else None, "extra": (0.5 * rnd(N, E, *HW)).to(dev) if E else None}
    index = torch.arange(FRAMES, device=dev).repeat(n_traj) if merge else None
    grad = rnd(N, C + E, *HW).to(dev, dtype)
    return t, index, grad


def baseline(t, n_traj):
    x = F.relu(F.group_norm(t["x"], GROUPS, t["weight"].to(t["x"].dtype), t["bias"].to(t["x"].dtype)))
    if t["skip"] is not None:
        cur = t["skip"].repeat(n_traj, 1, 1, 1)
        x = cur + F.interpolate(x, size=cur.shape[-2:], mode="nearest")
    if t["extra"] is not None:
        x = torch.cat([x, t["extra"].to(x.dtype)], 1)
    return x.permute(0, 2, 3, 1).contiguous()


def algorithmic_bytes(stage, N, dtype, backward):
    C, E, (h, w), (H, W), merge = stage
    es = torch.empty((), dtype=dtype).element_size()
    nx, nout, nskip, nextra = N * C * h * w, N * (C + E) * H * W, (FRAMES * C * H * W if merge else 0), N * E * H * W
    fwd = 2 * nx * es + nskip * es + nextra * 4 + nout * es
    if not backward:
        return fwd
    bwd = nout * es + 2 * nx * es + 2 * nx * 4 + nx * es + (N * C * H * W * es + nskip * es if merge else 0)
    return fwd + bwd


def stepper(fn, t, grad, backward):
    if not backward:
        def step():
            with torch.no_grad():
                fn(t)
        return step
    leaves = {k: (None if v is None else v.detach().requires_grad_(True)) for k, v in t.items()}
    live = [v for v in leaves.values() if v is not None]

    def step():
        torch.autograd.grad(fn(leaves), live, grad)
    return step


def window(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # microseconds per call


def measure(steps, windows, iters):
    for s in steps:
        for _ in range(3):
            s()
    torch.cuda.synchronize()
    times = ([], [])
    for _ in range(windows):        # alternating windows
        for t, s in zip(times, steps):
            t.append(window(s, iters))
    med = [statistics.median(t) for t in times]
    return {"operator_us": round(med[0], 2), "baseline_us": round(med[1], 2), "speedup": round(med[1] / med[0], 3),
            "faster_by_more_than_the_spread": bool(max(times[0]) < min(times[1])),
            "faster_in_the_median_only": bool(med[0] < med[1] and not max(times[0]) < min(times[1])),
            "operator_windows_us": [round(v, 2) for v in times[0]], "baseline_windows_us": [round(v, 2) for v in times[1]]}


def module_row(dev, windows, iters):
    """MaskHeadConv forward + backward at N = 60 on a 360x640 clip: this package's module against its own layers with the
    PyTorch glue (HIP convolutions on both sides)."""
    from devis_amd.modules import MaskHeadConv
    torch.manual_seed(0)
    m = MaskHeadConv(256, [256, 256, 256], 8, True, [0, 1, 2], 3).to(dev)
    sizes = [(12, 20), (23, 40), (45, 80), (90, 160)]
    n_traj = 10
    features = [torch.randn(FRAMES, 256, *s, device=dev) for s in sizes]
    maps = [0.5 * torch.randn(FRAMES * n_traj, 8, *s, device=dev) for s in sizes[:3]]
    expand = lambda t, n: t.repeat(n, 1, 1, 1)      # noqa: E731
    params = list(m.parameters())

    def theirs():
        x = torch.cat([expand(features[0], n_traj), maps[0]], 1)
        x = F.relu(m.gn1(m.lay1(x)))
        x = F.relu(m.gn2(m.lay2(x)))
        for lvl, feature in enumerate(features[1:]):
            cur = expand(getattr(m, "adapter%d" % (lvl + 1))(feature), n_traj)
            x = cur + F.interpolate(x, size=cur.shape[-2:], mode="nearest")
            if lvl + 1 < len(maps):
                x = torch.cat([x, maps[lvl + 1]], 1)
            x = F.relu(getattr(m, "gn%d" % (lvl + 3))(getattr(m, "lay%d" % (lvl + 3))(x)))
        return m.out_lay(x)

    def step_of(fn):
        def step():
            out = fn()
            torch.autograd.grad(out.sum(), params)
        return step

    row = measure([step_of(lambda: m(features, maps, n_traj, expand)), step_of(theirs)], windows, iters)
    row.update({"row": "MaskHeadConv", "N": FRAMES * n_traj, "dtype": "f32", "pass": "fwd+bwd", "clip": "360x640"})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maskhead_stage_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-module", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("maskhead_stage_bench needs the GPU: there is no CPU path to time")
    import devis_amd
    dev = torch.device("cuda:0")
    rows = []
    for dtype, label in ((torch.float32, "f32"), (torch.bfloat16, "bf16, f32 parameters and maps")):
        for stage in STAGES:
            for n_traj in TRAJECTORIES:
                t, index, grad = make(stage, n_traj, dtype, dev)
                ours = lambda t: devis_amd.mask_head_stage(t["x"], GROUPS, t["weight"], t["bias"], skip=t["skip"],      # noqa: E731
                                                           skip_index=index, extra=t["extra"])
                theirs = lambda t: baseline(t, n_traj)      # noqa: E731
                for backward in (False, True):
                    g = grad if backward else None
                    gb = None if g is None else g.permute(0, 2, 3, 1).contiguous()      # the baseline's result is NHWC
                    row = measure([stepper(ours, t, g, backward), stepper(theirs, t, gb, backward)], args.windows, args.iters)
                    nbytes = algorithmic_bytes(stage, FRAMES * n_traj, dtype, backward)
                    C, E, hw, HW, merge = stage
                    row.update({"row": "%d @ %dx%d -> %dx%d + %d" % (C, hw[0], hw[1], HW[0], HW[1], E), "N": FRAMES * n_traj,
                                "dtype": label, "pass": "fwd+bwd" if backward else "fwd", "algorithmic_bytes": nbytes,
                                "hbm_fraction": round(nbytes / (row["operator_us"] * 1e-6) / HBM_BYTES_PER_S, 4)})
                    rows.append(row)
                    print(json.dumps({k: row[k] for k in ("row", "N", "dtype", "pass", "operator_us", "baseline_us", "speedup",
                                                          "hbm_fraction", "faster_by_more_than_the_spread")}), flush=True)
    if not args.no_module:
        row = module_row(dev, args.windows, max(args.iters // 4, 3))
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("windows_us")}), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "windows": args.windows, "iters": args.iters,
           "method": "device events; median of alternating windows; every window kept", "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
