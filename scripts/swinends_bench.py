"""Times the two ends of a Swin backbone under devis_amd.patch_swin_ends against the stock modules, on the same GPU, in the same
process, on the same device tensors and parameters.  The modules are stand-ins with the reference's chain: a PatchEmbed (F.pad,
4 x 4 / stride-4 Conv2d, flatten + transpose, LayerNorm, transpose + view, followed by the flatten + transpose of
SwinTransformer.forward, so that both sides end with the token tensor) and an output norm (LayerNorm, view, permute,
contiguous), at Swin-L's shapes on a 6-frame clip at 800 x 1333:

    patch embed     [6, 3, 800, 1333] -> [6, 200 * 334, 192]
    output norms    [6, 200 * 334, 192], [6, 100 * 167, 384], [6, 50 * 84, 768], [6, 25 * 42, 1536]

float32, and float32 parameters and input under bfloat16 autocast; in eval mode (forward, no_grad) and in training mode
(forward + backward of every parameter, and of the input of an output norm).

    python scripts/swinends_bench.py [--out profiles/swinends_bench.json] [--windows 3] [--seconds 0.3]

Method (that of scripts/swinglue_bench.py): every side is warmed up.  "ms" is the call time: a window is `iters` calls between
two device events, `iters` chosen so that a window lasts at least `--seconds`; the windows of the two sides alternate; the
median is quoted and every window is kept.  "host_ms" is the host clock around the same calls without the synchronise.  In a run
of their own, per call: the device activities of a torch.profiler trace and their summed duration, this library's calls, and the
bytes the call newly allocates with the peak above the level before the call.  "least_bytes" is what one pass has to move,
computed from the shapes.  Nothing is measured on the CPU, and no ratio is fixed in advance: every row is reported, losing rows
included.
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

IMAGE = (6, 3, 800, 1333, 4, 192)                           # B, Cin, H, W, patch, embedding channels
NORMS = [(6, 200, 334, 192), (6, 100, 167, 384), (6, 50, 84, 768), (6, 25, 42, 1536)]      # B, H, W, C


class PatchEmbed(nn.Module):
    def __init__(self, patch_size, in_chans, embed_dim):
        super().__init__()
        self.patch_size, self.embed_dim = (patch_size, patch_size), embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        self.norm = nn.LayerNorm(embed_dim)

    def forward(self, x):
        H, W = x.shape[2:]
        if W % self.patch_size[1] != 0:
            x = F.pad(x, (0, self.patch_size[1] - W % self.patch_size[1]))
        if H % self.patch_size[0] != 0:
            x = F.pad(x, (0, 0, 0, self.patch_size[0] - H % self.patch_size[0]))
        x = self.proj(x)
        Wh, Ww = x.size(2), x.size(3)
        x = self.norm(x.flatten(2).transpose(1, 2))
        return x.transpose(1, 2).view(-1, self.embed_dim, Wh, Ww)


class SwinTransformer(nn.Module):
    """The exits of the backbone only: ``forward(x_out, H, W)`` is what the reference does with a stage's output."""
    def __init__(self, dim):
        super().__init__()
        self.num_features, self.out_indices, self.norm0 = [dim], (0,), nn.LayerNorm(dim)

    def forward(self, x_out, H, W):
        return self.norm0(x_out).view(-1, H, W, self.num_features[0]).permute(0, 3, 1, 2).contiguous()


def fused_exit(self, x_out, H, W):
    import devis_amd
    return devis_amd.layer_norm_to_map(x_out, H, W, self.norm0.weight, self.norm0.bias, self.norm0.eps)


def counts_of(fn):
    """SB.counts_of with this operator's launches."""
    from devis_amd import _swinends
    names = ("embed_forward", "embed_backward", "map_forward", "map_backward")
    originals = {name: getattr(_swinends, name) for name in names}
    launches = []
    for name, orig in originals.items():
        setattr(_swinends, name, lambda *a, _orig=orig: (launches.append(1), _orig(*a))[1])
    try:
        fn()
    finally:
        for name, orig in originals.items():
            setattr(_swinends, name, orig)
    res = SB.counts_of(fn)
    res["library_launches"] = len(launches)
    return res


def measure(rows, what, info, dtype_name, training, sides, leaves, grad, args):
    def run(fn):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype_name == "bfloat16 autocast"):
            return fn()
    if training:
        res = SB.compare({k: (lambda fn=fn: torch.autograd.grad(run(fn), leaves, grad)) for k, fn in sides.items()}, args.windows,
                         args.seconds, counts_of)
    else:
        with torch.no_grad():
            res = SB.compare({k: (lambda fn=fn: run(fn)) for k, fn in sides.items()}, args.windows, args.seconds, counts_of)
    row = dict(info, what=what, dtype=dtype_name, mode="training fwd+bwd" if training else "eval fwd", stock=res["stock"], fused=res["fused"])
    row["stock_over_fused"] = res["stock"]["ms"] / res["fused"]["ms"]
    rows.append(row)
    print("%-12s %-32s %-18s %-17s stock %8.3f ms  fused %8.3f ms  x%.2f  alloc %6.0f -> %6.0f MB" % (
        what, info["shape"], dtype_name, row["mode"], res["stock"]["ms"], res["fused"]["ms"], row["stock_over_fused"],
        res["stock"]["allocated_bytes"] / 1e6, res["fused"]["allocated_bytes"] / 1e6), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swinends_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("swinends_bench.py measures on the GPU; there is none here")
    import devis_amd
    from devis_amd.modules import swin_ends
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5)
    rows = []
    stand_in = types.SimpleNamespace(PatchEmbed=PatchEmbed, SwinTransformer=SwinTransformer)
    B, Cin, H, W, p, C = IMAGE
    embed = PatchEmbed(p, Cin, C).to(dev)
    image = torch.randn(B, Cin, H, W, generator=g).to(dev)
    L = -(-H // p) * -(-W // p)
    grad = torch.randn(B, L, C, generator=g).to(dev)
    tokens_of = lambda forward: forward(embed, image).flatten(2).transpose(1, 2)      # noqa: E731
    sides = {"stock": lambda: tokens_of(PatchEmbed.forward), "fused": lambda: tokens_of(swin_ends.embed_forward)}
    with torch.no_grad():
        a, b = sides["stock"](), sides["fused"]()
        assert b.is_contiguous() and float((a - b).abs().max()) <= 1e-4 * float(a.abs().max())
    info = {"shape": "[%d, %d, %d, %d] -> [%d, %d, %d]" % (B, Cin, H, W, B, L, C), "least_bytes": 4 * (B * Cin * H * W + B * L * C)}
    previous = devis_amd.patch_swin_ends(stand_in)          # (records the stock forwards the fused ones fall back to)
    try:
        sides = {"stock": lambda: tokens_of(previous["PatchEmbed"]), "fused": lambda: tokens_of(swin_ends.embed_forward)}
        for dtype_name in ("float32", "bfloat16 autocast"):
            for training in (False, True):
                measure(rows, "patch embed", info, dtype_name, training, sides, list(embed.parameters()), grad, args)
        del image, grad
        for B, H, W, C in NORMS:
            exits = SwinTransformer(C).to(dev)
            x = torch.randn(B, H * W, C, generator=g).to(dev).requires_grad_(True)
            grad = torch.randn(B, C, H, W, generator=g).to(dev)
            sides = {"stock": lambda: previous["SwinTransformer"](exits, x, H, W), "fused": lambda: fused_exit(exits, x, H, W)}
            with torch.no_grad():
                a, b = sides["stock"](), sides["fused"]()
                assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-4 * float(a.abs().max())
            info = {"shape": "[%d, %d * %d, %d] -> NCHW" % (B, H, W, C), "least_bytes": 8 * B * H * W * C}
            for dtype_name in ("float32", "bfloat16 autocast"):
                for training in (False, True):
                    measure(rows, "output norm", info, dtype_name, training, sides, [x] + list(exits.parameters()), grad, args)
            del x, grad
    finally:
        devis_amd.unpatch_swin_ends(stand_in, previous)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows, "seconds": args.seconds,
           "method": "alternating windows between device events, median; see the module docstring", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
