"""Times a Swin stage under devis_amd.patch_swin_glue against the same stage under devis_amd.patch_window_attention alone (the
route before the glue kernels), on the same GPU, in the same process, on the same device tensors and parameters.  The stage is a
stand-in with the reference's attribute names and chain: a BasicLayer of two blocks (scripts/winattn_bench.py's block with a
DropPath), shifts 0 and half the window, which builds the shift mask on every call as the reference does, and a PatchMerging:

    [6, 200 * 334, 192], 6 heads, window 7      the first Swin-L stage of a 6-frame clip at 800 x 1333
    [6, 25 * 42, 1536], 48 heads, window 7      the last stage
    [6, 100 * 167, 192], 6 heads, window 12     a window of 12 (N = 144)

and the PatchMerging alone at the first shape.  float32, and float32 parameters and input under bfloat16 autocast; in eval mode
(forward, no_grad) and in training mode with drop_path = 0.2 (forward + backward of the input and every parameter; both sides
start every call from the same generator seed, so they draw the same masks).

    python scripts/swinglue_bench.py [--out profiles/swinglue_bench.json] [--windows 3] [--seconds 0.3]

Method (that of scripts/winattn_bench.py): every side is warmed up.  "ms" is the call time: a window is `iters` calls between
two device events, `iters` chosen so that a window lasts at least `--seconds`; the windows of the two sides alternate; the
median is quoted and every window is kept.  "host_ms" is the host clock around the same calls without the synchronise.  In a run
of their own, per call: "device_ms", the sum of the durations of the device activities a torch.profiler trace lists, their
number, this library's calls, and the bytes the call newly allocates with the peak above the level before the call.  Nothing is
measured on the CPU, and no ratio is fixed in advance: every row is reported, losing rows included.
"""
import argparse
import json
import os
import sys
import types

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import selfattn_bench as SB  # noqa: E402
import winattn_bench as WB  # noqa: E402

SHAPES = WB.SHAPES                      # (B, H, W, C, heads, window)
DROP_PATH = 0.2


class DropPath(nn.Module):
    def __init__(self, drop_prob):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep_prob = 1 - self.drop_prob
        return x * x.new_empty((x.shape[0],) + (1,) * (x.ndim - 1)).bernoulli_(keep_prob).div_(keep_prob)


class Block(WB.StockBlock):
    def __init__(self, dim, heads, ws, shift, drop_path):
        super().__init__(dim, heads, ws, shift)
        self.mlp = Mlp(dim)
        self.drop_path = DropPath(drop_path) if drop_path > 0 else nn.Identity()


class Mlp(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.fc1, self.act, self.fc2 = nn.Linear(dim, 4 * dim), nn.GELU(), nn.Linear(4 * dim, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class Merging(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dim, self.reduction, self.norm = dim, nn.Linear(4 * dim, 2 * dim, bias=False), nn.LayerNorm(4 * dim)

    def forward(self, x, H, W):
        B, L, C = x.shape
        x = x.view(B, H, W, C)
        if H % 2 == 1 or W % 2 == 1:
            x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
        x = torch.cat([x[:, 0::2, 0::2, :], x[:, 1::2, 0::2, :], x[:, 0::2, 1::2, :], x[:, 1::2, 1::2, :]], -1)
        return self.reduction(self.norm(x.view(B, -1, 4 * C)))


class Layer(nn.Module):
    def __init__(self, block, dim, heads, ws, drop_path):
        super().__init__()
        self.window_size, self.shift_size, self.use_checkpoint, self.downsample = ws, ws // 2, False, None
        self.blocks = nn.ModuleList([block(dim, heads, ws, 0 if i % 2 == 0 else ws // 2, drop_path) for i in range(2)])

    def forward(self, x, H, W):
        ws, shift = self.window_size, self.shift_size
        Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
        img_mask = torch.zeros((1, Hp, Wp, 1), device=x.device)                  # the reference's mask, built on every call
        cuts = (slice(0, -ws), slice(-ws, -shift), slice(-shift, None))
        cnt = 0
        for h in cuts:
            for w in cuts:
                img_mask[:, h, w, :] = cnt
                cnt += 1
        mask_windows = WB.partition(img_mask, ws).view(-1, ws * ws)
        attn_mask = mask_windows.unsqueeze(1) - mask_windows.unsqueeze(2)
        attn_mask = attn_mask.masked_fill(attn_mask != 0, float(-100.0)).masked_fill(attn_mask == 0, float(0.0))
        for blk in self.blocks:
            blk.H, blk.W = H, W
            x = blk(x, attn_mask)
        return x, H, W, x, H, W


def module():
    """A namespace of fresh classes by the reference's names, to patch on its own."""
    return types.SimpleNamespace(**{name: type(name, (base,), {"forward": base.forward}) for name, base in (
        ("SwinTransformerBlock", Block), ("BasicLayer", Layer), ("PatchMerging", Merging))})


def counts_of(fn):
    """Per call of fn: device activities of a profiler trace and their summed duration, this library's calls, newly allocated
    bytes and their peak."""
    from devis_amd import _prenorm, _winattn
    calls = []
    originals = [(m, name, getattr(m, name)) for m in (_winattn, _prenorm) for name in ("forward", "backward")]
    for m, name, orig in originals:
        setattr(m, name, lambda *a, _orig=orig: calls.append(1) or _orig(*a))
    try:
        fn()
    finally:
        for m, name, orig in originals:
            setattr(m, name, orig)
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


def measure(rows, what, shape_info, dtype_name, training, sides, leaves, args, g, dev):
    """One row: ``sides`` {name: forward function} timed as eval forwards or as training forward + backwards."""
    autocast = lambda: torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype_name == "bfloat16 autocast")      # noqa: E731

    def forward(fn):
        torch.manual_seed(0)                                 # (both sides draw the same drop-path masks)
        with autocast():
            return fn()

    with torch.no_grad():
        outs = {k: forward(fn) for k, fn in sides.items()}
    difference = float((outs["window_attention"].float() - outs["swin_glue"].float()).abs().max())
    grad = torch.randn(outs["swin_glue"].shape, generator=g).to(device=dev, dtype=outs["swin_glue"].dtype)
    del outs
    if training:
        res = SB.compare({k: (lambda fn=fn, k=k: torch.autograd.grad(forward(fn), leaves[k], grad)) for k, fn in sides.items()},
                         args.windows, args.seconds)
    else:
        with torch.no_grad():
            res = SB.compare({k: (lambda fn=fn: forward(fn)) for k, fn in sides.items()}, args.windows, args.seconds)
    a, b = res["window_attention"], res["swin_glue"]
    rows.append(dict(shape_info, what=what, dtype=dtype_name, training=training, mode="forward_backward" if training else "forward",
                     drop_path=DROP_PATH if training else 0.0, max_difference=difference, before_over_after=a["ms"] / b["ms"],
                     before_over_after_host=a["host_ms"] / b["host_ms"], **res))
    fmt = lambda v: "%8.3f" % v if isinstance(v, float) else "%8s" % "n/m"      # noqa: E731
    print("%-6s %-16s ws %-2d %-18s %-5s before %8.3f ms (host %8.3f, device %s, %s activities, %d MiB new), after %8.3f ms (host "
          "%8.3f, device %s, %s activities, %d MiB new), ratio %.2f, max difference %.2e" % (
              what, "x".join(map(str, shape_info["shape"])), shape_info["window"], dtype_name, "train" if training else "eval",
              a["ms"], a["host_ms"], fmt(a["device_ms"]), a["device_activities"], a["allocated_bytes"] >> 20,
              b["ms"], b["host_ms"], fmt(b["device_ms"]), b["device_activities"], b["allocated_bytes"] >> 20,
              rows[-1]["before_over_after"], difference), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swinglue_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("swinglue_bench: no GPU; nothing is measured on the CPU")
    import devis_amd
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    SB.counts_of = counts_of                                # (compare() reports this library's calls)
    before, after = module(), module()
    devis_amd.patch_window_attention(before)
    devis_amd.patch_window_attention(after)
    devis_amd.patch_swin_glue(after)
    rows = []
    for index, (B, H, W, C, heads, ws) in enumerate(SHAPES):
        for dtype_name in ("float32", "bfloat16 autocast"):
            for training in (False, True):
                rate = DROP_PATH if training else 0.0
                stages = {"window_attention": before.BasicLayer(before.SwinTransformerBlock, C, heads, ws, rate),
                          "swin_glue": after.BasicLayer(after.SwinTransformerBlock, C, heads, ws, rate)}
                merges = {"window_attention": before.PatchMerging(C), "swin_glue": after.PatchMerging(C)}
                for group in (stages, merges):
                    for m in group.values():
                        m.to(dev).train(training)
                    group["swin_glue"].load_state_dict(group["window_attention"].state_dict())
                x = torch.randn(B, H * W, C, generator=g).to(dev).requires_grad_(training)
                info = {"shape": [B, H * W, C], "map": [H, W], "heads": heads, "window": ws}
                measure(rows, "stage", info, dtype_name, training, {k: (lambda m=m: m(x, H, W)[0]) for k, m in stages.items()},      # noqa: B023
                        {k: [x] + list(m.parameters()) for k, m in stages.items()}, args, g, dev)
                if index == 0:
                    measure(rows, "merge", info, dtype_name, training, {k: (lambda m=m: m(x, H, W)) for k, m in merges.items()},      # noqa: B023
                            {k: [x] + list(m.parameters()) for k, m in merges.items()}, args, g, dev)
                del stages, merges, x
                torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows, "seconds": args.seconds,
           "sides": {"window_attention": "devis_amd.patch_window_attention alone", "swin_glue": "devis_amd.patch_swin_glue on top"},
           "method": "ms: a window is `iters` calls between two device events, lasting at least `seconds`; windows of the two "
                     "sides alternate; medians quoted.  host_ms: the host clock around the same calls without the synchronise.  "
                     "Counts are per call, from a run of their own: device activities of a torch.profiler trace and the sum of "
                     "their durations (device_ms), this library's calls, bytes newly allocated and their peak above the level "
                     "before.  A whole-backbone or end-to-end figure was not measured",
           "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
