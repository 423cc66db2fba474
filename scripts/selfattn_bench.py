"""Times the decoder's query self-attention on devis_amd.FusedMultiheadAttention (patch_self_attention) against the stock
nn.MultiheadAttention it replaces, on the same GPU, in the same process, on the same device tensors and parameters:

    module  self_attn(q, k, tgt)[0] with q and k two views of one tensor, as the reference's decoder layer calls it
    layer   one stand-in decoder layer -- the reference's attribute names and chain, its cross attention a stub that returns a
            fixed tensor -- against the same layer under patch_self_attention AND patch_transformer_layers

for [300, 1, 256] and [300, 2, 256] ([queries, batch, channels]; 8 heads), float32 and bfloat16, in eval mode (forward,
no_grad) and in training mode (p = 0.1; forward + backward).

    python scripts/selfattn_bench.py [--out profiles/selfattn_bench.json] [--windows 3] [--seconds 0.3]

Method: every side is warmed up.  "ms" is the call time: a window is `iters` calls between two device events, `iters` chosen so
that a window lasts at least `--seconds`; the windows of the two sides alternate; the median is quoted and every window is kept.
"host_ms" is the host clock around the same `iters` calls WITHOUT the synchronise -- what the Python and the launches cost the
host --, measured in windows of its own that end in a synchronise outside the clock.  In a run of their own, per call:
"device_ms", the sum of the durations of the device activities a torch.profiler trace lists (kernels, copies, memsets; "not
measured" where the profiler gives none), their number, this library's launches, and the bytes the call newly allocates (the
allocator's cumulative counter) with the peak above the level before the call.  Nothing is measured on the CPU.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time
import types

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((300, 1, 256), (300, 2, 256))
HEADS, D_FFN, P_TRAIN = 8, 1024, 0.1


class StockDecoderLayer(nn.Module):
    """The attributes the patched methods read and the chain the reference's layer computes; ``cross_attn`` is set by the
    caller.  Tensors are batch-first, as the reference's are."""

    def __init__(self, d_model, d_ffn, dropout, n_heads):
        super().__init__()
        self.cross_attn = None
        self.dropout1, self.norm1 = nn.Dropout(dropout), nn.LayerNorm(d_model)
        self.self_attn = nn.MultiheadAttention(d_model, n_heads, dropout=dropout)
        self.dropout2, self.norm2 = nn.Dropout(dropout), nn.LayerNorm(d_model)
        self.linear1, self.activation, self.dropout3 = nn.Linear(d_model, d_ffn), F.relu, nn.Dropout(dropout)
        self.linear2, self.dropout4, self.norm3 = nn.Linear(d_ffn, d_model), nn.Dropout(dropout), nn.LayerNorm(d_model)

    @staticmethod
    def with_pos_embed(tensor, pos):
        return tensor if pos is None else tensor + pos

    def forward_ffn(self, tgt):
        hidden = self.dropout3(self.activation(self.linear1(tgt)))
        return self.norm3(tgt + self.dropout4(self.linear2(hidden)))

    def forward(self, tgt, query_pos, reference_points, src, src_spatial_shapes, level_start_index, **kwargs):
        q = k = self.with_pos_embed(tgt, query_pos)
        tgt2 = self.self_attn(q.transpose(0, 1), k.transpose(0, 1), tgt.transpose(0, 1))[0].transpose(0, 1)
        tgt = self.norm2(tgt + self.dropout2(tgt2))
        attended = self.cross_attn(self.with_pos_embed(tgt, query_pos), reference_points, src, src_spatial_shapes,
                                   level_start_index, **kwargs)[0]
        return self.forward_ffn(self.norm1(tgt + self.dropout1(attended)))


# ---- measuring -----------------------------------------------------------------------------------------------------------

def window(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def host_window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    elapsed = time.perf_counter() - t0
    torch.cuda.synchronize()
    return elapsed * 1e3 / iters


def counts_of(fn):
    """Per call of fn: device activities of a profiler trace and their summed duration, this library's launches, newly
    allocated bytes and their peak."""
    from devis_amd import _addnorm, _selfattn
    launches = []
    patched = []
    for module, names in ((_selfattn, ("forward", "backward")), (_addnorm, ("forward", "backward", "relu_forward", "relu_backward"))):
        for name in names:
            orig = getattr(module, name)
            patched.append((module, name, orig))

            def counted(*a, _orig=orig, _counts=module is _selfattn):
                rc = _orig(*a)
                launches.append(rc if _counts else 1)
                return rc
            setattr(module, name, counted)
    try:
        fn()
    finally:
        for module, name, orig in patched:
            setattr(module, name, orig)
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


def compare(sides, windows, seconds, counts=None):
    """{name: fn} -> {name: {"ms": median, "host_ms": median, "windows_ms": [...], "iters": n, counts}}, the sides' windows
    alternating.  ``counts`` replaces :func:`counts_of` for another operator's calls."""
    counts = counts or counts_of
    iters = {}
    for k, fn in sides.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        once = max(window(fn, 3), 1e-3)
        iters[k] = max(5, int(math.ceil(seconds * 1e3 / once)))
    times, host = {k: [] for k in sides}, {k: [] for k in sides}
    for _ in range(windows):
        for k, fn in sides.items():
            times[k].append(window(fn, iters[k]))
    for _ in range(windows):
        for k, fn in sides.items():
            host[k].append(host_window(fn, iters[k]))
    return {k: dict({"ms": statistics.median(times[k]), "host_ms": statistics.median(host[k]), "windows_ms": times[k],
                     "host_windows_ms": host[k], "iters": iters[k]}, **counts(fn)) for k, fn in sides.items()}


def subjects(shape, dtype, training, dev, g):
    """{subject: (stock side, fused side, stock leaves, fused leaves)}: callables of no arguments returning the result."""
    import devis_amd
    L, N, C = shape
    new = lambda *s: torch.randn(*s, generator=g).to(device=dev, dtype=dtype).requires_grad_(training)      # noqa: E731
    tgt, pos = new(N, L, C), new(N, L, C)                          # batch-first, as the decoder layer holds them
    stock_attn = nn.MultiheadAttention(C, HEADS, dropout=P_TRAIN).to(device=dev, dtype=dtype).train(training)
    fused_attn = nn.MultiheadAttention(C, HEADS, dropout=P_TRAIN).to(device=dev, dtype=dtype).train(training)
    fused_attn.load_state_dict(stock_attn.state_dict())
    devis_amd.patch_self_attention(fused_attn)
    q = (tgt + pos).detach().requires_grad_(training)

    def call(module):
        return lambda: module(q.transpose(0, 1), q.transpose(0, 1), tgt.transpose(0, 1))[0]

    out = {"module": (call(stock_attn), call(fused_attn), [q, tgt] + list(stock_attn.parameters()),
                      [q, tgt] + list(fused_attn.parameters()))}
    patched_class = type("DeformableTransformerDecoderLayer", (StockDecoderLayer,), {
        "forward": StockDecoderLayer.forward, "forward_ffn": StockDecoderLayer.forward_ffn})
    encoder_class = type("DeformableTransformerEncoderLayer", (StockDecoderLayer,), {
        "forward": StockDecoderLayer.forward, "forward_ffn": StockDecoderLayer.forward_ffn})      # (the patch wants both names)
    devis_amd.patch_transformer_layers(types.SimpleNamespace(DeformableTransformerEncoderLayer=encoder_class,
                                                             DeformableTransformerDecoderLayer=patched_class))
    stock = StockDecoderLayer(C, D_FFN, P_TRAIN, HEADS).to(device=dev, dtype=dtype).train(training)
    patched = patched_class(C, D_FFN, P_TRAIN, HEADS).to(device=dev, dtype=dtype).train(training)
    patched.load_state_dict(stock.state_dict())
    devis_amd.patch_self_attention(patched)
    attended = new(N, L, C)
    stock.cross_attn = patched.cross_attn = lambda *a, **k: (attended, None)
    out["layer"] = (lambda: stock(tgt, pos, None, None, None, None), lambda: patched(tgt, pos, None, None, None, None),
                    [tgt, attended] + list(stock.parameters()), [tgt, attended] + list(patched.parameters()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selfattn_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("selfattn_bench: no GPU; nothing is measured on the CPU")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rows = []
    for shape in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            for training in (False, True):
                for subject, (stock_side, fused_side, leaves, fused_leaves) in subjects(shape, dtype, training, dev, g).items():
                    with torch.no_grad():
                        a, b = stock_side(), fused_side()
                    # (in training mode the two sides draw different masks: only eval results are compared)
                    difference = None if training else float((a.float() - b.float()).abs().max())
                    grad = torch.randn(a.shape, generator=g).to(device=dev, dtype=a.dtype)
                    del a, b
                    if training:
                        mode = "forward_backward"
                        res = compare({"stock": lambda: torch.autograd.grad(stock_side(), leaves, grad),                  # noqa: B023
                                       "fused": lambda: torch.autograd.grad(fused_side(), fused_leaves, grad)},           # noqa: B023
                                      args.windows, args.seconds)
                    else:
                        mode = "forward"
                        with torch.no_grad():
                            res = compare({"stock": stock_side, "fused": fused_side}, args.windows, args.seconds)
                    rows.append({"subject": subject, "shape": list(shape), "dtype": str(dtype).replace("torch.", ""),
                                 "training": training, "mode": mode, "max_difference": difference,
                                 "stock_over_fused": res["stock"]["ms"] / res["fused"]["ms"],
                                 "stock_over_fused_host": res["stock"]["host_ms"] / res["fused"]["host_ms"], **res})
                    fmt = lambda v: "%8.3f" % v if isinstance(v, float) else "%8s" % "n/m"      # noqa: E731
                    print("%-6s %-11s %-8s %-5s stock %8.3f ms (host %8.3f, device %s, %s activities), fused %8.3f ms (host %8.3f, "
                          "device %s, %s activities), ratio %.2f" % (
                              subject, "x".join(map(str, shape)), rows[-1]["dtype"], "train" if training else "eval",
                              res["stock"]["ms"], res["stock"]["host_ms"], fmt(res["stock"]["device_ms"]), res["stock"]["device_activities"],
                              res["fused"]["ms"], res["fused"]["host_ms"], fmt(res["fused"]["device_ms"]), res["fused"]["device_activities"],
                              rows[-1]["stock_over_fused"]), flush=True)
                torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows, "seconds": args.seconds,
           "heads": HEADS, "d_ffn": D_FFN, "p_train": P_TRAIN,
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
