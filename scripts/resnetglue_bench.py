"""Times stand-in ResNet stages under devis_amd.patch_resnet_glue against the same stages unpatched (the stock route: the
reference's FrozenBatchNorm2d, in-place ReLUs, the shortcut add and nn.MaxPool2d), on the same GPU, in the same process, on the
same device tensors and parameters, with torch's own convolutions on both sides.  The stand-ins have torchvision's attribute
names and call order (tests/resnet_cases.py's, and a stem of the same kind):

    stem     conv 7x7/2, norm, ReLU, max-pool on [6, 3, 800, 1333]            (the norm sees [6, 64, 400, 667])
    layer1   a Bottleneck without downsample on [6, 256, 200, 334], planes 64
    layer4   a Bottleneck without downsample on [6, 2048, 25, 42], planes 512

in float32 and under bfloat16 autocast (keep_input_dtype off and on), contiguous NCHW and channels-last, as eval forward
(no_grad) and as training forward + backward of the convolution weights and the input (the stem is frozen, as in the
reference: its training row is the same forward with autograd recording, and has no backward).

    python scripts/resnetglue_bench.py [--out profiles/resnetglue_bench.json] [--windows 3] [--seconds 0.2]

Method (that of scripts/swinglue_bench.py): every side is warmed up.  "ms" is the call time: a window is `iters` calls between
two device events, `iters` chosen so that a window lasts at least `--seconds`; the windows of the two sides alternate; the
median is quoted and every window is kept.  In a run of their own, per call: the device activities of a torch.profiler trace
and the sum of their durations, this library's calls, and the newly allocated bytes with their peak.  No ratio is fixed in
advance: every row is reported, losing rows included.  Nothing is measured on the CPU.

The fused kernels alone, against the HBM peak:

    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/resnetglue_bench.py --fused-calls DIR/manifest.json
    python scripts/resnetglue_bench.py --merge DIR [--out profiles/resnetglue_bench.json]

The first issues the fused calls of the rows' shapes alone, in a known order, and writes that order with the bytes every call
reads and writes (computed from the shapes); the second matches the trace's frozennorm dispatches to it in order and adds
"kernels" to the JSON: bytes over the median kernel time, as a fraction of HBM_PEAK.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

sys.path.insert(0, os.path.join(ROOT, "tests"))

import resnet_cases as R  # noqa: E402  (the stand-ins the tests use: one copy)
import selfattn_bench as SB  # noqa: E402

HBM_PEAK = 8.0e12           # bytes / s: the MI355X's HBM3E peak
CLIP = 6
ROWS = (("stem", (CLIP, 3, 800, 1333)), ("layer1", (CLIP, 256, 200, 334)), ("layer4", (CLIP, 2048, 25, 42)))
MODES = (("float32", False, False), ("bfloat16 autocast", True, False), ("bfloat16 autocast, keep_input_dtype", True, True))


class Stem(nn.Module):
    """The stem alone, with torchvision's attribute names; frozen, as in the reference."""

    def __init__(self):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False), R.FrozenBatchNorm2d(64)
        self.relu, self.maxpool = nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.conv1.weight.requires_grad_(False)

    def forward(self, x):
        return self.maxpool(self.relu(self.bn1(self.conv1(x))))


def counts_of(fn):
    """Per call of fn: device activities of a profiler trace and their summed duration, this library's calls, newly allocated
    bytes and their peak."""
    from devis_amd import _frozennorm
    calls = []
    originals = [(name, getattr(_frozennorm, name)) for name in ("forward", "backward", "pool_forward")]
    for name, orig in originals:
        setattr(_frozennorm, name, lambda *a, _orig=orig: calls.append(1) or _orig(*a))
    try:
        fn()
    finally:
        for name, orig in originals:
            setattr(_frozennorm, name, orig)
    torch.cuda.synchronize()
    key = "allocated_bytes.all.allocated"
    before_total, before_level = torch.cuda.memory_stats()[key], torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_stats()[key] - before_total
    peak = torch.cuda.max_memory_allocated() - before_level
    activities = device_ms = "not measured"
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        events = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        if events:
            activities, device_ms = len(events), sum(e.time_range.elapsed_us() for e in events) / 1e3
    except Exception as exc:        # (a profiler that cannot trace here must not stop the timing)
        activities = device_ms = "not measured: %s" % type(exc).__name__
    return {"device_activities": activities, "device_ms": device_ms, "library_calls": len(calls), "allocated_bytes": allocated,
            "peak_bytes": peak}


def stage_of(row, dev, seed):
    model = Stem() if row == "stem" else (R.Bottleneck(256, 64) if row == "layer1" else R.Bottleneck(2048, 512))
    assert row == "stem" or model.downsample is None
    return R.randomise(model, seed).float().to(dev)


def measure(args):
    import copy

    import devis_amd
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rows = []
    for row, shape in ROWS:
        for layout in ("NCHW", "channels_last"):
            memory_format = torch.channels_last if layout == "channels_last" else torch.contiguous_format
            stock = stage_of(row, dev, len(row)).to(memory_format=memory_format)
            x = torch.randn(shape, generator=g).to(dev).contiguous(memory_format=memory_format)
            for dtype_name, autocast, keep in MODES:
                fused = copy.deepcopy(stock)
                devis_amd.patch_resnet_glue(fused, keep_input_dtype=keep)
                for training in (False, True):
                    xs = x.detach().requires_grad_(training and row != "stem")
                    sides = {"stock": stock, "resnet_glue": fused}

                    def forward(m):
                        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                            return m(xs)                     # noqa: B023

                    with torch.no_grad():
                        outs = {k: forward(m) for k, m in sides.items()}
                    difference = float((outs["stock"].float() - outs["resnet_glue"].float()).abs().max())
                    out_max = float(outs["stock"].float().abs().max())
                    grads = {k: torch.randn(o.shape, generator=g).to(dev, o.dtype).contiguous(memory_format=memory_format) for k, o in outs.items()}
                    del outs
                    if training and row != "stem":
                        leaves = {k: [xs] + [p for p in m.parameters() if p.requires_grad] for k, m in sides.items()}
                        res = SB.compare({k: (lambda m=m, k=k: torch.autograd.grad(forward(m), leaves[k], grads[k])) for k, m in sides.items()},      # noqa: B023
                                         args.windows, args.seconds, counts_of)
                    elif training:
                        res = SB.compare({k: (lambda m=m: forward(m)) for k, m in sides.items()}, args.windows, args.seconds, counts_of)      # noqa: B023
                    else:
                        with torch.no_grad():
                            res = SB.compare({k: (lambda m=m: forward(m)) for k, m in sides.items()}, args.windows, args.seconds, counts_of)      # noqa: B023
                    a, b = res["stock"], res["resnet_glue"]
                    rows.append(dict(row=row, shape=list(shape), layout=layout, dtype=dtype_name, training=training,
                                     mode=("forward_backward" if row != "stem" else "forward_recording") if training else "forward",
                                     max_difference=difference, output_max=out_max, stock_over_fused=a["ms"] / b["ms"], **res))
                    fmt = lambda v: "%8.3f" % v if isinstance(v, float) else "%8s" % "n/m"      # noqa: E731
                    print("%-6s %-13s %-36s %-5s stock %8.3f ms (device %s, %s activities, %d MiB new), fused %8.3f ms (device %s, %s "
                          "activities, %d MiB new), ratio %.3f, max difference %.2e of %.2e" % (
                              row, layout, dtype_name, "train" if training else "eval", a["ms"], fmt(a["device_ms"]),
                              a["device_activities"], a["allocated_bytes"] >> 20, b["ms"], fmt(b["device_ms"]), b["device_activities"],
                              b["allocated_bytes"] >> 20, rows[-1]["stock_over_fused"], difference, out_max), flush=True)
                    del grads, xs
                del fused
                torch.cuda.empty_cache()
            del stock, x
            torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows, "seconds": args.seconds,
           "sides": {"stock": "the stand-in stage as it is", "resnet_glue": "a copy under devis_amd.patch_resnet_glue"},
           "method": "ms: a window is `iters` calls between two device events, lasting at least `seconds`; windows of the two "
                     "sides alternate; medians quoted.  host_ms: the host clock around the same calls without the synchronise.  "
                     "Counts are per call, from a run of their own: device activities of a torch.profiler trace and the sum of "
                     "their durations (device_ms), this library's calls, bytes newly allocated and their peak above the level "
                     "before.  A whole-backbone or end-to-end figure was not measured",
           "results": rows}
    write(args.out, doc)


def write(path, doc):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", path)


# ---- the fused kernels alone ------------------------------------------------------------------------------------------------

def fused_calls(path, repeats=5):
    """Issues the fused calls of the rows' shapes alone, ``repeats`` times each after one warm-up, and writes their order."""
    import devis_amd
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    f32, bf16 = torch.float32, torch.bfloat16
    size = lambda *ts: sum(t.numel() * t.element_size() for t in ts if t is not None)      # noqa: E731
    manifest = []
    for row, shape in (("stem", (CLIP, 64, 400, 667)), ("layer1", (CLIP, 256, 200, 334)), ("layer4", (CLIP, 2048, 25, 42))):
        C = shape[1]
        norm = [t.to(dev) for t in (torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g))]
        for layout in ("NCHW", "channels_last"):
            memory_format = torch.channels_last if layout == "channels_last" else torch.contiguous_format
            for x_dtype, r_dtype, y_dtype in ((f32, f32, f32), (bf16, f32, f32), (bf16, bf16, bf16)):
                x = torch.randn(shape, generator=g).to(dev, x_dtype).contiguous(memory_format=memory_format)
                names = "%s/%s/%s" % tuple(str(d).replace("torch.", "") for d in (x_dtype, r_dtype, y_dtype))
                entries = []
                if row == "stem":
                    call = lambda: devis_amd.frozen_batch_norm_relu_pool(x, *norm, out_dtype=y_dtype)      # noqa: E731,B023
                    entries.append(("pool", call, lambda y: size(x, y)))      # noqa: B023
                else:
                    r = torch.randn(shape, generator=g).to(dev, r_dtype).contiguous(memory_format=memory_format)
                    entries.append(("norm_relu", lambda: devis_amd.frozen_batch_norm(x, *norm, relu=True, out_dtype=y_dtype), lambda y: size(x, y)))      # noqa: B023
                    entries.append(("norm_add_relu", lambda: devis_amd.frozen_batch_norm(x, *norm, residual=r, relu=True, out_dtype=y_dtype), lambda y: size(x, r, y)))      # noqa: B023

                    def backward():
                        xs, rs = x.detach().requires_grad_(True), r.detach().requires_grad_(True)      # noqa: B023
                        y = devis_amd.frozen_batch_norm(xs, *norm, residual=rs, relu=True, out_dtype=y_dtype)      # noqa: B023
                        torch.autograd.grad(y, [xs, rs], y)       # (grad_y = y: one more tensor is not needed)
                        return y
                    # a backward call is one forward dispatch and one backward dispatch: both are listed
                    entries.append(("norm_add_relu+backward", backward, lambda y: (size(x, r, y), size(y, x, r))))      # noqa: B023
                with torch.no_grad() if row == "stem" else torch.enable_grad():
                    for what, call, nbytes in entries:
                        for i in range(repeats + 1):
                            y = call()
                            sizes = nbytes(y)
                            for j, b in enumerate(sizes if isinstance(sizes, tuple) else (sizes,)):
                                manifest.append({"row": row, "shape": list(shape), "layout": layout, "dtypes": names,
                                                 "what": what.split("+")[0] if j == 0 else "backward", "warmup": i == 0, "bytes": b})
                            del y
                torch.cuda.synchronize()
    write(path, {"calls": manifest})


def merge(directory, out):
    """Matches the frozennorm dispatches of the kernel trace under ``directory`` to the manifest, in order."""
    with open(os.path.join(directory, "manifest.json")) as f:
        manifest = json.load(f)["calls"]
    traces = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if len(traces) != 1:
        raise SystemExit("resnetglue_bench: expected one kernel trace under %s, found %d" % (directory, len(traces)))
    with open(traces[0], newline="") as f:
        dispatches = [d for d in csv.DictReader(f) if "frozennorm" in d["Kernel_Name"]]
    dispatches.sort(key=lambda d: int(d["Start_Timestamp"]))
    if len(dispatches) != len(manifest):
        raise SystemExit("resnetglue_bench: %d frozennorm dispatches for %d calls" % (len(dispatches), len(manifest)))
    groups = {}
    for call, d in zip(manifest, dispatches):
        if not call["warmup"]:
            key = (call["row"], call["layout"], call["dtypes"], call["what"])
            groups.setdefault(key, dict(call, ns=[], kernel=d["Kernel_Name"].split("(")[0]))["ns"].append(int(d["End_Timestamp"]) - int(d["Start_Timestamp"]))
    kernels = []
    for group in groups.values():
        ns = statistics.median(group.pop("ns"))
        group.pop("warmup")
        rate = group["bytes"] / (ns * 1e-9)
        kernels.append(dict(group, kernel_us=ns / 1e3, bytes_per_second=rate, fraction_of_hbm_peak=rate / HBM_PEAK))
        print("%-6s %-13s %-26s %-14s %9.1f us %6.2f TB/s %5.1f %% of peak" % (group["row"], group["layout"], group["dtypes"], group["what"],
                                                                           ns / 1e3, rate / 1e12, 100 * rate / HBM_PEAK))
    with open(out) as f:
        doc = json.load(f)
    doc["hbm_peak_bytes_per_second"] = HBM_PEAK
    doc["kernels"] = kernels
    write(out, doc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnetglue_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.2)
    ap.add_argument("--fused-calls", metavar="MANIFEST")
    ap.add_argument("--merge", metavar="DIR")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    if not torch.cuda.is_available():
        raise SystemExit("resnetglue_bench: no GPU; nothing is measured on the CPU")
    if args.fused_calls:
        return fused_calls(args.fused_calls)
    measure(args)


if __name__ == "__main__":
    main()
