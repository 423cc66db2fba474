"""Records tests/golden/maskhead_*.npz from the REFERENCE's MaskHeadConv (src/models/deformable_segmentation.py) with plain
convolutions (use_deformable_conv=False: torchvision is not needed), in float64 on the CPU: a randomised state dict, the
features, the attention maps, the output, and the gradients of every input and parameter for a recorded grad_out.

    python tests/golden/make_golden_maskhead.py [/path/to/reference]

The smallest constructible head: dim=64, nheads=8, fpn_dims=[24], two attention-map levels, num_levels=2 -- GroupNorms over
72, 32 and 16 channels, one merge stage with extra channels and one plain stage; maps of 3x5 and 7x9; F = 2 frames, 3
instances, N = 6.  Two cases: DeVIS's ``tensor.repeat(n, 1, 1, 1)`` expansion and the image model's interleaved one.
Parameters and inputs are drawn exact in float16 and stored so (about 75 k parameters); results are float64.  Tensors only.
"""
import os

import numpy as np
import torch

from make_golden_attmap import import_reference_segmentation

HERE = os.path.dirname(os.path.abspath(__file__))
DIM, HEADS, FPN, FRAMES, INSTANCES = 64, 8, [24], 2, 3
MAPS = [(3, 5), (7, 9)]
CASES = {"maskhead_repeat": "repeat", "maskhead_interleaved": "interleaved"}


def expand_for(kind):
    if kind == "repeat":        # DeVIS (src/models/devis_segmentation.py)
        return lambda t, n: t.repeat(n, 1, 1, 1)
    return lambda t, n: t.unsqueeze(1).repeat(1, int(n), 1, 1, 1).flatten(0, 1)       # the image model


def main():
    seg = import_reference_segmentation()
    torch.set_default_dtype(torch.float64)
    for seed, (name, kind) in enumerate(sorted(CASES.items())):
        g = torch.Generator().manual_seed(2000 + seed)
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).half().double()      # noqa: E731
        m = seg.MaskHeadConv(DIM, FPN, HEADS, False, [0, 1], 2).double()
        with torch.no_grad():
            for pn, p in m.named_parameters():
                if ".weight" in pn and p.dim() == 4:
                    p.copy_((rnd(*p.shape) * (p[0].numel() ** -0.5)).half().double())
                elif pn.startswith("gn") and pn.endswith("weight"):
                    p.copy_((1 + 0.5 * rnd(*p.shape)).half().double())
                else:
                    p.copy_((0.3 * rnd(*p.shape)).half().double())
        N = FRAMES * INSTANCES
        features = [rnd(FRAMES, DIM, *MAPS[0]).requires_grad_(True), rnd(FRAMES, FPN[0], *MAPS[1]).requires_grad_(True)]
        bbox_mask = [(0.5 * rnd(N, HEADS, h, w)).half().double().requires_grad_(True) for h, w in MAPS]
        out = m(features, bbox_mask, INSTANCES, expand_for(kind))
        go = rnd(*out.shape)
        params = dict(m.named_parameters())
        leaves = features + bbox_mask + list(params.values())
        grads = torch.autograd.grad(out, leaves, go)
        d = {"out": out, "grad_out": go.half()}
        for i in range(2):
            d["feature/%d" % i], d["grad/feature/%d" % i] = features[i].half(), grads[i]
            d["bbox_mask/%d" % i], d["grad/bbox_mask/%d" % i] = bbox_mask[i].half(), grads[2 + i]
        for (pn, p), gp in zip(params.items(), grads[4:]):
            assert torch.equal(p.half().double(), p.detach())
            d["state/" + pn], d["grad/state/" + pn] = p.half(), gp
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **{k: v.detach().numpy() for k, v in d.items()})
        print("wrote %s: %d arrays, %d bytes" % (name, len(d), os.path.getsize(os.path.join(HERE, name + ".npz"))))


if __name__ == "__main__":
    main()
