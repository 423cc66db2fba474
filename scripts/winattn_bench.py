"""Times a Swin block under devis_amd.patch_window_attention against the stock block it replaces, on the same GPU, in the same
process, on the same device tensors and parameters.  The block is a stand-in with the reference's attribute names and chain
(norm1, pad, roll, window partition, qkv, logits, relative-position bias, shift mask, softmax, product with v, proj, window
reverse, roll, slice, shortcut, MLP), with a shift of half the window:

    [6, 200 * 334, 192], 6 heads, window 7      the first Swin-L stage of a 6-frame clip at 800 x 1333
    [6, 25 * 42, 1536], 48 heads, window 7      the last stage
    [6, 100 * 167, 192], 6 heads, window 12     a window of 12 (N = 144)

float32 and bfloat16 (parameters and input in that dtype), in eval mode (forward, no_grad) and in training mode (forward +
backward of the input and every parameter).

    python scripts/winattn_bench.py [--out profiles/winattn_bench.json] [--windows 3] [--seconds 0.3]

Method (that of scripts/selfattn_bench.py, whose helpers this imports): every side is warmed up.  "ms" is the call time: a
window is `iters` calls between two device events, `iters` chosen so that a window lasts at least `--seconds`; the windows of the
two sides alternate; the median is quoted and every window is kept.  "host_ms" is the host clock around the same calls without
the synchronise.  In a run of their own, per call: "device_ms", the sum of the durations of the device activities a
torch.profiler trace lists, their number, this library's launches, and the bytes the call newly allocates with the peak above
the level before the call.  Nothing is measured on the CPU.
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

# (B, H, W, C, heads, window)
SHAPES = ((6, 200, 334, 192, 6, 7), (6, 25, 42, 1536, 48, 7), (6, 100, 167, 192, 6, 12))
MASKED = -100.0


def relative_rows(ws):
    t = torch.arange(ws * ws)
    y, x = t // ws, t % ws
    return (y[:, None] - y[None, :] + ws - 1) * (2 * ws - 1) + (x[:, None] - x[None, :] + ws - 1)


def partition(x, ws):
    B, Hp, Wp, C = x.shape
    return x.view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)


def reverse(windows, ws, Hp, Wp):
    C = windows.shape[-1]
    return windows.view(-1, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, Hp, Wp, C)


def shift_mask(Hp, Wp, ws, shift, device, dtype):
    regions = torch.zeros(1, Hp, Wp, 1)
    cuts = (slice(0, -ws), slice(-ws, -shift), slice(-shift, None))
    for number, (rows, cols) in enumerate((r, c) for r in cuts for c in cuts):
        regions[:, rows, cols] = number
    per_window = partition(regions, ws)[..., 0]
    return ((per_window[:, :, None] != per_window[:, None, :]).float() * MASKED).to(device=device, dtype=dtype)


class Attention(nn.Module):
    def __init__(self, dim, ws, heads):
        super().__init__()
        self.dim, self.window_size, self.num_heads, self.scale = dim, (ws, ws), heads, (dim // heads) ** -0.5
        self.relative_position_bias_table = nn.Parameter(torch.randn((2 * ws - 1) ** 2, heads) * 0.02)
        self.register_buffer("relative_position_index", relative_rows(ws))
        self.qkv, self.proj = nn.Linear(dim, 3 * dim), nn.Linear(dim, dim)
        self.attn_drop, self.proj_drop = nn.Dropout(0.0), nn.Dropout(0.0)

    def forward(self, x, mask=None):
        windows, N, C = x.shape
        H = self.num_heads
        q, k, v = self.qkv(x).reshape(windows, N, 3, H, C // H).permute(2, 0, 3, 1, 4)
        logits = (q * self.scale) @ k.transpose(-2, -1)
        bias = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(N, N, H).permute(2, 0, 1).contiguous()
        logits = logits + bias.unsqueeze(0)
        if mask is not None:
            per_map = mask.shape[0]
            logits = (logits.view(windows // per_map, per_map, H, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, H, N, N)
        x = (self.attn_drop(torch.softmax(logits, -1)) @ v).transpose(1, 2).reshape(windows, N, C)
        return self.proj_drop(self.proj(x))


class StockBlock(nn.Module):
    def __init__(self, dim, heads, ws, shift):
        super().__init__()
        self.window_size, self.shift_size = ws, shift
        self.norm1, self.attn, self.norm2 = nn.LayerNorm(dim), Attention(dim, ws, heads), nn.LayerNorm(dim)
        self.drop_path = nn.Identity()
        self.mlp = nn.Sequential(nn.Linear(dim, 4 * dim), nn.GELU(), nn.Linear(4 * dim, dim))
        self.H = self.W = None

    def forward(self, x, mask_matrix):
        B, L, C = x.shape
        H, W, ws, shift = self.H, self.W, self.window_size, self.shift_size
        shortcut = x
        x = F.pad(self.norm1(x).view(B, H, W, C), (0, 0, 0, -W % ws, 0, -H % ws))
        Hp, Wp = x.shape[1:3]
        shifted = torch.roll(x, (-shift, -shift), (1, 2)) if shift else x
        windows = self.attn(partition(shifted, ws), mask=mask_matrix if shift else None)
        shifted = reverse(windows, ws, Hp, Wp)
        x = torch.roll(shifted, (shift, shift), (1, 2)) if shift else shifted
        x = x[:, :H, :W, :].contiguous().view(B, H * W, C)
        x = shortcut + self.drop_path(x)
        return x + self.drop_path(self.mlp(self.norm2(x)))


def counts_of(fn):
    """Per call of fn: device activities of a profiler trace and their summed duration, this library's launches, newly
    allocated bytes and their peak."""
    from devis_amd import _winattn
    launches = []
    originals = {name: getattr(_winattn, name) for name in ("forward", "backward")}
    for name, orig in originals.items():
        setattr(_winattn, name, lambda *a, _orig=orig: launches.append(_orig(*a)) or launches[-1])
    try:
        fn()
    finally:
        for name, orig in originals.items():
            setattr(_winattn, name, orig)
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
    return {"device_activities": activities, "device_ms": device_ms, "library_launches": sum(launches), "allocated_bytes": allocated,
            "peak_bytes": peak}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "winattn_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("winattn_bench: no GPU; nothing is measured on the CPU")
    import devis_amd
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    SB.counts_of = counts_of                                # (compare() reports this library's launches)
    fused_class = type("SwinTransformerBlock", (StockBlock,), {"forward": StockBlock.forward})
    devis_amd.patch_window_attention(types.SimpleNamespace(SwinTransformerBlock=fused_class))
    rows = []
    for B, H, W, C, heads, ws in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            for training in (False, True):
                stock = StockBlock(C, heads, ws, ws // 2).to(device=dev, dtype=dtype).train(training)
                fused = fused_class(C, heads, ws, ws // 2).to(device=dev, dtype=dtype).train(training)
                fused.load_state_dict(stock.state_dict())
                stock.H = fused.H = H
                stock.W = fused.W = W
                x = torch.randn(B, H * W, C, generator=g).to(device=dev, dtype=dtype).requires_grad_(training)
                mask = shift_mask(H + -H % ws, W + -W % ws, ws, ws // 2, dev, dtype)
                stock_side, fused_side = (lambda: stock(x, mask)), (lambda: fused(x, mask))      # noqa: B023
                with torch.no_grad():
                    a, b = stock_side(), fused_side()
                difference = float((a.float() - b.float()).abs().max())
                grad = torch.randn(a.shape, generator=g).to(device=dev, dtype=a.dtype)
                del a, b
                if training:
                    mode = "forward_backward"
                    leaves, fused_leaves = [x] + list(stock.parameters()), [x] + list(fused.parameters())
                    res = SB.compare({"stock": lambda: torch.autograd.grad(stock_side(), leaves, grad),                  # noqa: B023
                                      "fused": lambda: torch.autograd.grad(fused_side(), fused_leaves, grad)},           # noqa: B023
                                     args.windows, args.seconds)
                else:
                    mode = "forward"
                    with torch.no_grad():
                        res = SB.compare({"stock": stock_side, "fused": fused_side}, args.windows, args.seconds)
                rows.append({"shape": [B, H * W, C], "map": [H, W], "heads": heads, "window": ws, "shift": ws // 2,
                             "dtype": str(dtype).replace("torch.", ""), "training": training, "mode": mode,
                             "max_difference": difference, "stock_over_fused": res["stock"]["ms"] / res["fused"]["ms"],
                             "stock_over_fused_host": res["stock"]["host_ms"] / res["fused"]["host_ms"], **res})
                fmt = lambda v: "%8.3f" % v if isinstance(v, float) else "%8s" % "n/m"      # noqa: E731
                print("%-14s ws %-2d %-8s %-5s stock %8.3f ms (host %8.3f, device %s, %s activities, %d MiB new), fused %8.3f ms "
                      "(host %8.3f, device %s, %s activities, %d MiB new), ratio %.2f, max difference %.2e" % (
                          "x".join(map(str, (B, H * W, C))), ws, rows[-1]["dtype"], "train" if training else "eval",
                          res["stock"]["ms"], res["stock"]["host_ms"], fmt(res["stock"]["device_ms"]), res["stock"]["device_activities"],
                          res["stock"]["allocated_bytes"] >> 20,
                          res["fused"]["ms"], res["fused"]["host_ms"], fmt(res["fused"]["device_ms"]), res["fused"]["device_activities"],
                          res["fused"]["allocated_bytes"] >> 20, rows[-1]["stock_over_fused"], difference), flush=True)
                del stock, fused, x, mask, grad
                torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows, "seconds": args.seconds,
           "method": "ms: a window is `iters` calls between two device events, lasting at least `seconds`; windows of the two "
                     "sides alternate; medians quoted.  host_ms: the host clock around the same calls without the synchronise.  "
                     "Counts are per call, from a run of their own: device activities of a torch.profiler trace and the sum of "
                     "their durations (device_ms), this library's launches, bytes newly allocated and their peak above the "
                     "level before",
           "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
