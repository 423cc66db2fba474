"""Times the glue between the transformer layers' GEMMs on devis_amd.add_layer_norm / devis_amd.relu_dropout
(patch_transformer_layers) against the torch statement it replaces, on the same GPU, in the same process, on the same device
tensors:

    site    one norm site            F.layer_norm(x + F.dropout(delta, p))            against add_layer_norm
    ffn     the FFN's middle         F.dropout(F.relu(h), p), h [.., d_ffn]           against relu_dropout
    layer   an encoder layer's glue  a stand-in layer -- the reference's attribute names and chain, its attention a stub that
                                     returns a fixed tensor, so two norm sites, the FFN's middle and the two Linears -- against
                                     the same layer under patch_transformer_layers

for [6, 2540, 256] (the training clip), [6, 22223, 256] (800 x 1333) and [1, 300, 256] (the decoder's queries), d_ffn = 1024,
float32 and bfloat16, in training mode (p = 0.1; forward, and forward + backward) and in eval mode (forward, no_grad).

    python scripts/addnorm_bench.py [--out profiles/addnorm_bench.json] [--windows 3] [--seconds 0.3]

Method: every side is warmed up; a window is `iters` calls between two device events, `iters` chosen so that a window lasts at
least `--seconds`; the windows of the two sides alternate; the median is quoted and every window is kept.  In a run of their
own, per call: the device activities a torch.profiler trace lists (kernels, copies, memsets; "not measured" where the profiler
gives none), this library's launches, and the bytes the call newly allocates (the allocator's cumulative counter) with the
peak above the level before the call.  Nothing is measured on the CPU.
"""
import argparse
import json
import math
import os
import statistics
import sys
import types

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((6, 2540, 256), (6, 22223, 256), (1, 300, 256))
D_FFN = 1024
P_TRAIN = 0.1


class StockEncoderLayer(nn.Module):
    """The attributes the patched methods read and the chain the reference's layer computes; ``self_attn`` is set by the caller."""

    def __init__(self, d_model, d_ffn, dropout):
        super().__init__()
        self.self_attn = None
        self.dropout1, self.norm1 = nn.Dropout(dropout), nn.LayerNorm(d_model)
        self.linear1, self.activation, self.dropout2 = nn.Linear(d_model, d_ffn), F.relu, nn.Dropout(dropout)
        self.linear2, self.dropout3, self.norm2 = nn.Linear(d_ffn, d_model), nn.Dropout(dropout), nn.LayerNorm(d_model)

    @staticmethod
    def with_pos_embed(tensor, pos):
        return tensor if pos is None else tensor + pos

    def forward_ffn(self, src):
        hidden = self.dropout2(self.activation(self.linear1(src)))
        return self.norm2(src + self.dropout3(self.linear2(hidden)))

    def forward(self, src, pos, reference_points, spatial_shapes, level_start_index, **kwargs):
        attended = self.self_attn(self.with_pos_embed(src, pos), reference_points, src, spatial_shapes, level_start_index, **kwargs)[0]
        return self.forward_ffn(self.norm1(src + self.dropout1(attended)))


# ---- measuring -----------------------------------------------------------------------------------------------------------

def window(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def counts_of(fn):
    """Per call of fn: device activities of a profiler trace, this library's launches, newly allocated bytes and their peak."""
    from devis_amd import _addnorm
    launches = []
    names = ("forward", "backward", "relu_forward", "relu_backward")
    originals = {name: getattr(_addnorm, name) for name in names}
    for name, orig in originals.items():
        setattr(_addnorm, name, lambda *a, _orig=orig, _name=name: launches.append(_name) or _orig(*a))
    try:
        fn()
    finally:
        for name, orig in originals.items():
            setattr(_addnorm, name, orig)
    torch.cuda.synchronize()
    key = "allocated_bytes.all.allocated"
    before_total, before_level = torch.cuda.memory_stats()[key], torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_stats()[key] - before_total
    peak = torch.cuda.max_memory_allocated() - before_level
    activities = "not measured"
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        activities = n if n else "not measured"
    except Exception as exc:        # (a profiler that cannot trace here must not stop the timing)
        activities = "not measured: %s" % type(exc).__name__
    return {"device_activities": activities, "library_launches": len(launches), "allocated_bytes": allocated, "peak_bytes": peak}


def compare(sides, windows, seconds):
    """{name: fn} -> {name: {"ms": median, "windows_ms": [...], "iters": n, counts}}, the sides' windows alternating."""
    iters = {}
    for k, fn in sides.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        once = max(window(fn, 3), 1e-3)
        iters[k] = max(5, int(math.ceil(seconds * 1e3 / once)))
    times = {k: [] for k in sides}
    for _ in range(windows):
        for k, fn in sides.items():
            times[k].append(window(fn, iters[k]))
    return {k: dict({"ms": statistics.median(times[k]), "windows_ms": times[k], "iters": iters[k]}, **counts_of(fn))
            for k, fn in sides.items()}


def subjects(shape, dtype, training, dev, g):
    """{subject: (torch side, fused side, differentiable tensors)}: callables of no arguments returning the result."""
    import devis_amd
    T, S, C = shape
    p = P_TRAIN if training else 0.0
    new = lambda *s: torch.randn(*s, generator=g).to(device=dev, dtype=dtype).requires_grad_(training)      # noqa: E731
    x, delta, hidden = new(T, S, C), new(T, S, C), new(T, S, D_FFN)
    weight, bias = new(C), new(C)
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    out = {"site": (lambda: F.layer_norm(x + F.dropout(delta, p, training), (C,), weight, bias),
                    lambda: devis_amd.add_layer_norm(x, delta, weight, bias, p=p, seed=seed if p else None),
                    [x, delta, weight, bias]),
           "ffn": (lambda: F.dropout(F.relu(hidden), p, training),
                   lambda: devis_amd.relu_dropout(hidden, p=p, seed=seed if p else None), [hidden])}
    patched_class = type("DeformableTransformerEncoderLayer", (StockEncoderLayer,), {
        "forward": StockEncoderLayer.forward, "forward_ffn": StockEncoderLayer.forward_ffn})
    decoder_class = type("DeformableTransformerDecoderLayer", (StockEncoderLayer,), {
        "forward": StockEncoderLayer.forward, "forward_ffn": StockEncoderLayer.forward_ffn})      # (the patch wants both names)
    devis_amd.patch_transformer_layers(types.SimpleNamespace(DeformableTransformerEncoderLayer=patched_class,
                                                             DeformableTransformerDecoderLayer=decoder_class))
    stock = StockEncoderLayer(C, D_FFN, P_TRAIN).to(device=dev, dtype=dtype).train(training)
    patched = patched_class(C, D_FFN, P_TRAIN).to(device=dev, dtype=dtype).train(training)
    patched.load_state_dict(stock.state_dict())
    attended = new(T, S, C)
    stock.self_attn = patched.self_attn = lambda *a, **k: (attended, None)
    params = [x, attended] + list(stock.parameters())
    out["layer"] = (lambda: stock(x, None, None, None, None), lambda: patched(x, None, None, None, None),
                    params, [x, attended] + list(patched.parameters()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "addnorm_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("addnorm_bench: no GPU; nothing is measured on the CPU")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rows = []
    for shape in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            for training in (True, False):
                for subject, entry in subjects(shape, dtype, training, dev, g).items():
                    torch_side, fused_side, leaves = entry[:3]
                    fused_leaves = entry[3] if len(entry) > 3 else leaves
                    with torch.no_grad():
                        a, b = torch_side(), fused_side()
                    # (in training mode the two sides draw different masks: only eval results are compared)
                    difference = None if training else float((a.float() - b.float()).abs().max())
                    grad = torch.randn(a.shape, generator=g).to(device=dev, dtype=a.dtype)
                    del a, b
                    modes = {"forward": (torch_side, fused_side)}
                    if training:
                        modes["forward_backward"] = (lambda: torch.autograd.grad(torch_side(), leaves, grad),              # noqa: B023
                                                     lambda: torch.autograd.grad(fused_side(), fused_leaves, grad))        # noqa: B023
                    for mode, (replaced, fused) in modes.items():
                        if training:
                            res = compare({"replaced": replaced, "fused": fused}, args.windows, args.seconds)
                        else:
                            with torch.no_grad():
                                res = compare({"replaced": replaced, "fused": fused}, args.windows, args.seconds)
                        rows.append({"subject": subject, "shape": list(shape), "dtype": str(dtype).replace("torch.", ""),
                                     "training": training, "mode": mode, "max_difference": difference,
                                     "replaced_over_fused": res["replaced"]["ms"] / res["fused"]["ms"], **res})
                        print("%-5s %-16s %-8s %-5s %-16s replaced %8.3f ms, fused %8.3f ms, ratio %.2f" % (
                            subject, "x".join(map(str, shape)), rows[-1]["dtype"], "train" if training else "eval", mode,
                            res["replaced"]["ms"], res["fused"]["ms"], rows[-1]["replaced_over_fused"]), flush=True)
                torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows, "seconds": args.seconds,
           "d_ffn": D_FFN, "p_train": P_TRAIN,
           "method": "a window is `iters` calls between two device events, lasting at least `seconds`; windows of the two sides "
                     "alternate; medians quoted; counts are per call, from a run of their own: device activities of a "
                     "torch.profiler trace, this library's launches, bytes newly allocated and their peak above the level before",
           "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
