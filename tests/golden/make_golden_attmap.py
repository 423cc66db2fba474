"""Records tests/golden/attmap_*.npz from the REFERENCE's MultiScaleMHAttentionMap (src/models/deformable_segmentation.py),
in float64 on the CPU: randomised state dicts, the inputs, the per-level outputs, and the gradients of q, every k and every
parameter for a recorded grad_out.  Tensors only; a few kilobytes each.

    python tests/golden/make_golden_attmap.py [/path/to/reference]

The reference module is imported as make_golden.py imports the transformer: a package whose __init__ is skipped, with
torchvision and the module's sibling imports (none of which MultiScaleMHAttentionMap uses) as empty stand-ins.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"


class _Anything(types.ModuleType):
    """A stand-in module: any attribute is a placeholder class (enough for `from x import Y` and for base classes)."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (torch.nn.Module,), {})


def import_reference_segmentation():
    src = os.path.join(REFERENCE, "src")
    top = types.ModuleType("refsrc"); top.__path__ = [src]; sys.modules["refsrc"] = top
    pkg = types.ModuleType("refsrc.models"); pkg.__path__ = [os.path.join(src, "models")]; sys.modules["refsrc.models"] = pkg
    for name in ("torchvision", "torchvision.ops", "refsrc.util", "refsrc.util.misc", "refsrc.util.box_ops",
                 "refsrc.models.deformable_detr", "refsrc.models.deformable_transformer", "refsrc.models.ops",
                 "refsrc.models.ops.modules", "refsrc.models.backbone", "refsrc.models.matcher",
                 "refsrc.models.position_encoding", "refsrc.models.criterion", "refsrc.models.devis_ablation_segmentation"):
        sys.modules.setdefault(name, _Anything(name))
    return importlib.import_module("refsrc.models.deformable_segmentation")


CASES = {   # name -> (with mask, bias)
    "attmap_masked": (True, True),
    "attmap_nomask": (False, True),
    "attmap_nobias": (True, False),
}
B, Q, DIM, HIDDEN, HEADS = 2, 5, 8, 32, 4
PYRAMID = [(2, 3), (3, 5), (5, 7)]


def main():
    seg = import_reference_segmentation()
    torch.set_default_dtype(torch.float64)
    for seed, (name, (with_mask, bias)) in enumerate(sorted(CASES.items())):
        g = torch.Generator().manual_seed(1000 + seed)
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
        # (the reference's constructor zeroes the biases it was told not to create, so bias=False cannot be built there:
        # the case without biases takes them out of a module built with them; its forward handles None)
        m = seg.MultiScaleMHAttentionMap(DIM, HIDDEN, HEADS, len(PYRAMID), dropout=0, bias=True).double()
        if not bias:
            for layer in m.children():
                if isinstance(layer, torch.nn.Linear):
                    layer.register_parameter("bias", None)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(rnd(*p.shape) * (0.6 if p.dim() == 2 else 0.3))
        q = rnd(B, Q, DIM).requires_grad_(True)
        ks = [rnd(B, DIM, h, w).requires_grad_(True) for h, w in PYRAMID]
        masks = None
        if with_mask:   # padding masks: image 1 keeps the top-left ~3/4 of every map
            masks = []
            for h, w in PYRAMID:
                mk = torch.zeros(B, h, w, dtype=torch.bool)
                mk[1, :, w - max(1, w // 4):] = True
                mk[1, h - max(1, h // 4):, :] = True
                masks.append(mk)
        outs = m(q, ks, masks)
        gos = [rnd(*o.shape) for o in outs]
        params = dict(m.named_parameters())
        leaves = [q] + ks + list(params.values())
        grads = torch.autograd.grad(outs, leaves, gos)
        d = {"q": q, "grad/q": grads[0]}
        for i in range(len(PYRAMID)):
            d["k/%d" % i], d["out/%d" % i], d["grad_out/%d" % i], d["grad/k/%d" % i] = ks[i], outs[i], gos[i], grads[1 + i]
            if masks is not None:
                d["mask/%d" % i] = masks[i]
        for (pn, p), gp in zip(params.items(), grads[1 + len(PYRAMID):]):
            d["state/" + pn], d["grad/state/" + pn] = p, gp
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **{k: v.detach().numpy() for k, v in d.items()})
        print("wrote %s: %d arrays" % (name, len(d)))


if __name__ == "__main__":
    main()
