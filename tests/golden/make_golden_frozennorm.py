"""Records tests/golden/frozennorm.npz from the REFERENCE's FrozenBatchNorm2d (src/models/backbone.py), in float64 on the CPU:
a randomised state dict, a small input and the output.  Tensors only; a few kilobytes.

    python tests/golden/make_golden_frozennorm.py [/path/to/reference]

The reference module is imported as make_golden_attmap.py imports the mask head: a package whose __init__ is skipped, with
torchvision and the module's sibling imports (none of which FrozenBatchNorm2d uses) as empty stand-ins.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
N, C, H, W = 2, 6, 5, 7


class _Anything(types.ModuleType):
    """A stand-in module: any attribute is a placeholder class (enough for `from x import Y` and for base classes)."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (torch.nn.Module,), {})


def import_reference_backbone():
    src = os.path.join(REFERENCE, "src")
    top = types.ModuleType("refsrc"); top.__path__ = [src]; sys.modules["refsrc"] = top
    pkg = types.ModuleType("refsrc.models"); pkg.__path__ = [os.path.join(src, "models")]; sys.modules["refsrc.models"] = pkg
    for name in ("torchvision", "torchvision.models", "torchvision.models._utils", "refsrc.util", "refsrc.util.misc",
                 "refsrc.models.swin_backbone", "refsrc.models.position_encoding"):
        sys.modules.setdefault(name, _Anything(name))
    return importlib.import_module("refsrc.models.backbone")


def main():
    backbone = import_reference_backbone()
    g = torch.Generator().manual_seed(2301)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    m = backbone.FrozenBatchNorm2d(C).double()
    state = {"weight": rnd(C), "bias": rnd(C), "running_mean": rnd(C),
             "running_var": 0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64),
             "num_batches_tracked": torch.tensor(7)}       # (a BatchNorm2d checkpoint's extra key, which the module drops)
    m.load_state_dict(dict(state))
    x = 8 * torch.rand(N, C, H, W, generator=g, dtype=torch.float64) - 4
    d = {"x": x, "out": m(x)}
    for k, v in state.items():
        d["state/" + k] = v
    np.savez_compressed(os.path.join(HERE, "frozennorm.npz"), **{k: v.detach().numpy() for k, v in d.items()})
    print("wrote frozennorm: %d arrays" % len(d))


if __name__ == "__main__":
    main()
