"""Times the encoder's input projections under devis_amd.patch_input_proj against the stock modules, on the same GPU, in the same
process, on the same device tensors and parameters.  The projections are stand-ins with the reference's chain: four levels of
Conv2d + GroupNorm(32, 256) -- three 1 x 1 and a last 3 x 3 / stride 2 on the last feature map -- followed by prepare_data's
flatten(2).transpose(1, 2) per level and cat, so that both sides end with src_flatten.  Shapes:

    a 6-frame clip at 800 x 1333      levels 100 x 167, 50 x 84, 25 x 42, 13 x 21 (22 223 tokens)
    a training-sized clip             levels 34 x 56, 17 x 28, 9 x 14, 5 x 7 (2 541 tokens)

float32, and float32 parameters under bfloat16 autocast; in eval mode (forward, no_grad) and in training mode (forward +
backward of every parameter and feature); "norm" rows time the operator alone on the convolutions' outputs, "proj" rows the
convolutions with it.

    python scripts/inputproj_bench.py [--out profiles/inputproj_bench.json] [--windows 3] [--seconds 0.3]

Method: that of scripts/swinends_bench.py (alternating windows between device events, medians, every window kept; device
activities, this library's calls and newly allocated bytes from a run of their own).  No ratio is fixed in advance: every row is
reported, losing rows included.
"""
import argparse
import json
import os
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import selfattn_bench as SB  # noqa: E402

CLIPS = {"6 x 800 x 1333": (6, [(100, 167), (50, 84), (25, 42)]), "training clip": (6, [(34, 56), (17, 28), (9, 14)])}
CHANNELS, HIDDEN = (512, 1024, 2048), 256


class Projections(nn.Module):
    def __init__(self):
        super().__init__()
        layers = [nn.Sequential(nn.Conv2d(c, HIDDEN, kernel_size=1), nn.GroupNorm(32, HIDDEN)) for c in CHANNELS]
        layers.append(nn.Sequential(nn.Conv2d(CHANNELS[-1], HIDDEN, kernel_size=3, stride=2, padding=1), nn.GroupNorm(32, HIDDEN)))
        self.input_proj = nn.ModuleList(layers)

    def convolutions(self, features):
        return [self.input_proj[l][0](f) for l, f in enumerate(features)] + [self.input_proj[3][0](features[-1])]

    def norms(self, maps):
        from devis_amd.argument_builders import flatten_sources
        return flatten_sources([proj[1](x) for proj, x in zip(self.input_proj, maps)])

    def forward(self, features):
        return self.norms(self.convolutions(features))


def counts_of(fn):
    """SB.counts_of with this operator's launches."""
    from devis_amd import _inputproj
    originals = {name: getattr(_inputproj, name) for name in ("forward", "backward")}
    launches = []
    for name, orig in originals.items():
        setattr(_inputproj, name, lambda *a, _orig=orig: (launches.append(1), _orig(*a))[1])
    try:
        fn()
    finally:
        for name, orig in originals.items():
            setattr(_inputproj, name, orig)
    res = SB.counts_of(fn)
    res["library_launches"] = len(launches)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inputproj_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("inputproj_bench.py measures on the GPU; there is none here")
    import devis_amd
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5)
    rows = []
    model = Projections().to(dev)
    for clip, (N, sizes) in CLIPS.items():
        features = [torch.randn(N, c, h, w, generator=g).to(dev).requires_grad_(True) for c, (h, w) in zip(CHANNELS, sizes)]
        with torch.no_grad():
            maps = [m.requires_grad_(True) for m in model.convolutions(features)]
        tokens = sum(m.shape[2] * m.shape[3] for m in maps)
        grad = torch.randn(N, tokens, HIDDEN, generator=g).to(dev)
        norm_params = [p for proj in model.input_proj for p in proj[1].parameters()]

        def side(fn, patched):
            def call():
                previous = devis_amd.patch_input_proj(model) if patched else None
                try:
                    return fn()
                finally:
                    if patched:
                        devis_amd.unpatch_input_proj(model, previous)
            return call
        for what, fn, leaves in (("norm", lambda: model.norms(maps), maps + norm_params),
                                 ("proj", lambda: model(features), features + list(model.parameters()))):
            sides = {"stock": side(fn, False), "fused": side(fn, True)}
            with torch.no_grad():
                a, b = sides["stock"](), sides["fused"]()
                assert b.is_contiguous() and float((a - b).abs().max()) <= 1e-4 * float(a.abs().max())
            for dtype_name in ("float32", "bfloat16 autocast"):
                if what == "norm" and dtype_name != "float32":
                    continue                                # (the operator alone sees 16-bit maps only behind the convolutions)
                for training in (False, True):
                    def run(f):
                        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype_name == "bfloat16 autocast"):
                            return f()
                    if training:
                        res = SB.compare({k: (lambda f=f: torch.autograd.grad(run(f), leaves, grad)) for k, f in sides.items()},
                                         args.windows, args.seconds, counts_of)
                    else:
                        with torch.no_grad():
                            res = SB.compare({k: (lambda f=f: run(f)) for k, f in sides.items()}, args.windows, args.seconds, counts_of)
                    row = {"clip": clip, "tokens": tokens, "what": what, "dtype": dtype_name,
                           "mode": "training fwd+bwd" if training else "eval fwd", "stock": res["stock"], "fused": res["fused"],
                           "stock_over_fused": res["stock"]["ms"] / res["fused"]["ms"]}
                    rows.append(row)
                    print("%-16s %-5s %-18s %-17s stock %8.3f ms  fused %8.3f ms  x%.2f  alloc %6.0f -> %6.0f MB" % (
                        clip, what, dtype_name, row["mode"], res["stock"]["ms"], res["fused"]["ms"], row["stock_over_fused"],
                        res["stock"]["allocated_bytes"] / 1e6, res["fused"]["allocated_bytes"] / 1e6), flush=True)
        del features, maps, grad
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows, "seconds": args.seconds,
           "method": "alternating windows between device events, median; see the module docstring", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
