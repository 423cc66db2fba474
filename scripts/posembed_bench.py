"""Times the encoder's positional input on devis_amd.encoder_position_embedding against the formulation it replaces, on the
same GPU, in the same process: from the padding masks of all levels, the temporal and the level embedding to
lvl_pos_embed_flatten, mask_flatten and valid_ratios -- forward, and forward + backward to the two embeddings' gradients.

The replaced side is a restatement, in this script, of what the stock code computes with torch operators: per level
PositionEmbeddingSine's two cumsums, normalisations, divisions by dim_t, sin / cos on strided halves, stacks, cat and permute,
`+ temporal_embed`, `.to(dtype)`, then prepare_data's flatten / transpose / `+ level_embed[lvl]` / cat, get_valid_ratio per
level and the cat of the flattened masks.  Both sides get the same device tensors and must return the same embedding within
1e-4, and equal masks and valid ratios.

Shapes: the encoder shape the README quotes (800 x 1333, T = 6, C = 256, levels 100x167, 50x84, 25x42, 13x21) and one
training-sized clip (T = 6, C = 256, levels 38x50, 19x25, 10x13, 5x7).

Beside the times, per call: the ATen operators dispatched, the kernel launches of this library, the device activities a
torch.profiler trace lists ("not measured" where the profiler gives none), and the bytes newly allocated on the device
(torch.cuda.max_memory_allocated over a call, above the level before it).

    python scripts/posembed_bench.py [--out profiles/posembed_bench.json] [--windows 7] [--iters 20]

Method: every side is warmed up; a window is `iters` calls between a device synchronise and a host clock read after another
one; the windows of the sides alternate; the median of the windows is quoted and every window is kept.  Numbers are written
only by a run on an MI355X.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, CHANNELS = 6, 256
SHAPES = {"encoder 800x1333": [(100, 167), (50, 84), (25, 42), (13, 21)], "training clip": [(38, 50), (19, 25), (10, 13), (5, 7)]}


# ---- the replaced formulation, restated -------------------------------------------------------------------------------------

def stock_sine(mask, num_pos_feats, temperature=10000, scale=2 * math.pi):
    """The stock class's operator sequence (normalised), operator for operator: two cumsums and normalisations, one new table
    of periods per call, per axis the division, sin and cos on strided halves, stack and flatten; then cat and permute."""
    open_pixels = ~mask
    coordinates = [open_pixels.cumsum(axis, dtype=torch.float32) for axis in (1, 2)]
    coordinates = [c / (c.narrow(axis, c.shape[axis] - 1, 1) + 1e-6) * scale for axis, c in zip((1, 2), coordinates)]
    k = torch.arange(num_pos_feats, dtype=torch.float32, device=mask.device)
    periods = temperature ** (2 * (torch.div(k, 2, rounding_mode='trunc')) / num_pos_feats)
    halves = []
    for coordinate in coordinates:
        angle = coordinate[..., None] / periods
        halves.append(torch.stack((angle[..., 0::2].sin(), angle[..., 1::2].cos()), dim=-1).flatten(-2))
    return torch.cat(halves, dim=3).permute(0, 3, 1, 2)


def stock_valid_ratio(mask):
    open_pixels = ~mask
    rows, cols = torch.sum(open_pixels[:, :, 0], 1), torch.sum(open_pixels[:, 0, :], 1)
    return torch.stack([cols.float() / mask.shape[2], rows.float() / mask.shape[1]], -1)


def stock(masks, level_embed, temporal_embed, dtype=torch.float32):
    embeds = []
    for lvl, mask in enumerate(masks):
        pos = (stock_sine(mask, level_embed.shape[1] // 2) + temporal_embed[:, :, None, None]).to(dtype)
        embeds.append(pos.flatten(2).transpose(1, 2) + level_embed[lvl].view(1, 1, -1))
    return (torch.cat(embeds, 1), torch.cat([m.flatten(1) for m in masks], 1), torch.stack([stock_valid_ratio(m) for m in masks], 1))


# ---- measuring -----------------------------------------------------------------------------------------------------------

def window(fn, iters):
    torch.cuda.synchronize()
    start = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - start) * 1e3 / iters


class _Count(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def counts_of(fn):
    """Per call of fn: ATen operators dispatched, this library's kernel launches (a forward call is two, a backward call
    two), device activities of a profiler trace, bytes newly allocated."""
    from devis_amd import _posembed
    launches = []
    per_call = {"counts": 1, "write_flat": 1, "write_nchw": 1, "backward": 2}
    originals = {name: getattr(_posembed, name) for name in per_call}
    for name, orig in originals.items():
        setattr(_posembed, name, lambda *a, _orig=orig, _name=name: launches.append(per_call[_name]) or _orig(*a))
    try:
        with _Count() as mode:
            fn()
    finally:
        for name, orig in originals.items():
            setattr(_posembed, name, orig)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    allocated = torch.cuda.max_memory_allocated() - before
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
    return {"aten_calls": mode.n, "library_launches": sum(launches), "device_activities": activities,
            "newly_allocated_bytes": int(allocated)}


def compare(sides, windows, iters):
    """{name: fn} -> {name: {"ms": median, "windows_ms": [...], counts}}, the sides' windows alternating."""
    for fn in sides.values():
        for _ in range(5):
            fn()
    times = {k: [] for k in sides}
    for _ in range(windows):
        for k, fn in sides.items():
            times[k].append(window(fn, iters))
    return {k: dict({"ms": statistics.median(times[k]), "windows_ms": times[k]}, **counts_of(fn)) for k, fn in sides.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posembed_bench.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("posembed_bench: no GPU; nothing is measured on the CPU")
    import devis_amd
    dev = torch.device("cuda:0")
    name, arch = torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    g = torch.Generator().manual_seed(0)
    rows = []
    for label, sizes in SHAPES.items():
        masks = []
        for h, w in sizes:                              # every frame padded at the right and the bottom, by its own amount
            m = torch.zeros(FRAMES, h, w, dtype=torch.bool)
            for n in range(FRAMES):
                m[n, h - int(torch.randint(0, h // 4 + 1, (1,), generator=g)):, :] = True
                m[n, :, w - int(torch.randint(0, w // 4 + 1, (1,), generator=g)):] = True
            masks.append(m.to(dev))
        level = torch.randn(len(sizes), CHANNELS, generator=g).to(dev).requires_grad_(True)
        temporal = torch.randn(FRAMES, CHANNELS, generator=g).to(dev).requires_grad_(True)
        tokens = sum(h * w for h, w in sizes)
        weight = torch.randn(FRAMES, tokens, CHANNELS, generator=g).to(dev)

        def fused():
            return devis_amd.encoder_position_embedding(masks, level, temporal)                  # noqa: B023

        def replaced():
            return stock(masks, level, temporal)                                                 # noqa: B023

        def with_backward(fn):
            return lambda: torch.autograd.grad(fn()[0], (level, temporal), weight)              # noqa: B023

        with torch.no_grad():
            a, b = replaced(), fused()
        diff = float((a[0] - b[0]).abs().max())
        ga, gb = with_backward(replaced)(), with_backward(fused)()
        grad_diff = max(float(((x - y).abs() / x.abs().max()).max()) for x, y in zip(ga, gb))

        def no_grad(fn):
            def call():
                with torch.no_grad():
                    return fn()
            return call

        fwd = compare({"replaced": no_grad(replaced), "fused": no_grad(fused)}, args.windows, args.iters)
        both = compare({"replaced": with_backward(replaced), "fused": with_backward(fused)}, args.windows, args.iters)
        rows.append({"shape": label, "levels": sizes, "frames": FRAMES, "channels": CHANNELS, "tokens": tokens,
                     "output_bytes": FRAMES * tokens * CHANNELS * 4, "max_difference": diff, "same_embedding": diff <= 1e-4,
                     "same_masks_and_ratios": bool(torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])),
                     "max_relative_gradient_difference": grad_diff,
                     "forward": dict(fwd, replaced_over_fused=fwd["replaced"]["ms"] / fwd["fused"]["ms"]),
                     "forward_backward": dict(both, replaced_over_fused=both["replaced"]["ms"] / both["fused"]["ms"])})
        print("%s: forward replaced %.3f ms, fused %.3f ms; forward + backward replaced %.3f ms, fused %.3f ms"
              % (label, fwd["replaced"]["ms"], fwd["fused"]["ms"], both["replaced"]["ms"], both["fused"]["ms"]), flush=True)
    doc = {"device": name, "arch": arch, "torch": torch.__version__, "windows": args.windows, "iters": args.iters,
           "method": "a window is `iters` calls between device synchronises, by a host clock; windows of the sides alternate; "
                     "medians quoted; counts are per call: ATen operators by torch's dispatch mode, this library's kernel launches, "
                     "device activities of a torch.profiler trace, bytes newly allocated by torch.cuda.max_memory_allocated",
           "encoder_position_embedding": rows}
    if arch != "gfx950":            # (the MI355X's; the runtime may name the card generically)
        raise SystemExit("posembed_bench: %s (%s) is not an MI355X; the numbers are not recorded" % (name, arch))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
