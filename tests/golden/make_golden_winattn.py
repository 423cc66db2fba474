"""Records tests/golden/winattn_layer*.npz from the REFERENCE's own BasicLayer (src/models/swin_backbone.py), in float64 on the
CPU and in eval mode: dim 16, depth 2 (one block without a shift, one with a shift of 2), 2 heads, window 4, mlp_ratio 2, every
drop rate 0, no downsample; input [2, 6 * 9, 16] with H = 6 and W = 9, so the padded map is 8 x 12 and the stage pads, rolls,
masks and slices.  Tensors only; each file under 32 KiB.

    python tests/golden/make_golden_winattn.py /path/to/reference

The reference module is imported as make_golden_layerglue.py imports it -- a package whose __init__ is skipped, with stand-ins
for what the imports pull in and never call here -- plus a small stand-in for ``timm.models.layers``: ``DropPath`` (never built
at a drop rate of 0), ``to_2tuple`` and ``trunc_normal_`` (torch's own).

``winattn_layer`` holds the input ``x``, the state dict (``state.*``) and ``grad_out`` -- values exact in float16, stored in
float16; the index buffers as they are.  ``winattn_layer_out`` holds the float64 ``out`` and ``grad.x``.  The float64 gradients
of the parameters have files of their own, one per block: ``winattn_layer_grads_block0`` and ``winattn_layer_grads_block1``.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else None
LAYER = dict(dim=16, depth=2, num_heads=2, window_size=4, mlp_ratio=2.0)
B, H, W = 2, 6, 9


class _Anything(types.ModuleType):
    """A stand-in module: any attribute is a placeholder class (enough for `from x import Y`)."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def timm_layers():
    """What swin_backbone.py takes from timm.models.layers."""
    layers = types.ModuleType("timm.models.layers")

    class DropPath(torch.nn.Module):
        def __init__(self, drop_prob=0.0):
            super().__init__()
            assert drop_prob == 0.0, "the recorded stage has no stochastic depth"

        def forward(self, x):
            return x

    layers.DropPath = DropPath
    layers.to_2tuple = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    layers.trunc_normal_ = torch.nn.init.trunc_normal_
    return layers


def import_reference():
    src = os.path.join(REFERENCE, "src")
    for name, path in (("refsrc", src), ("refsrc.models", os.path.join(src, "models")), ("refsrc.util", os.path.join(src, "util"))):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    for name in ("timm", "timm.models", "refsrc.util.misc"):
        sys.modules.setdefault(name, _Anything(name))
    sys.modules["timm.models.layers"] = timm_layers()
    swin = importlib.import_module("refsrc.models.swin_backbone")
    assert swin.__file__ == os.path.join(src, "models", "swin_backbone.py")
    return swin


def exact16(*shape, generator):
    """float64 values that float16 holds exactly."""
    return torch.randn(*shape, generator=generator).to(torch.float16).double()


def fill(layer, generator):
    """Parameters exact in float16; the norms away from (1, 0) and the bias table away from 0.02 so that each matters."""
    with torch.no_grad():
        for name, p in layer.named_parameters():
            scale = 0.25 if p.dim() > 1 and "table" not in name else 1.0
            offset = 1.0 if ".norm" in name and name.endswith("weight") else 0.0
            p.copy_((exact16(*p.shape, generator=generator) * scale + offset).to(torch.float16).double())


def main():
    if REFERENCE is None:
        raise SystemExit(__doc__)
    swin = import_reference()
    g = torch.Generator().manual_seed(2101)
    layer = swin.BasicLayer(qkv_bias=True, qk_scale=None, drop=0.0, attn_drop=0.0, drop_path=0.0, norm_layer=torch.nn.LayerNorm,
                            downsample=None, use_checkpoint=False, **LAYER).double().eval()
    assert [blk.shift_size for blk in layer.blocks] == [0, 2]
    fill(layer, g)
    x = exact16(B, H * W, LAYER["dim"], generator=g).requires_grad_(True)
    grad_out = exact16(B, H * W, LAYER["dim"], generator=g)
    out = layer(x, H, W)[0]
    params = dict(layer.named_parameters())
    grads = torch.autograd.grad(out, [x] + list(params.values()), grad_out)
    half = lambda t: t.detach().to(torch.float16).numpy()      # noqa: E731
    for t in [x, grad_out] + list(params.values()):
        assert torch.equal(t.detach().to(torch.float16).double(), t.detach()), "not exact in float16"
    main_file = {"x": half(x), "grad_out": half(grad_out)}
    for name, t in layer.state_dict().items():
        main_file["state." + name] = half(t) if t.is_floating_point() else t.numpy()
    files = {"winattn_layer": main_file, "winattn_layer_out": {"out": out.detach().numpy(), "grad.x": grads[0].numpy()},
             "winattn_layer_grads_block0": {}, "winattn_layer_grads_block1": {}}
    for name, grad in zip(params, grads[1:]):
        block = name.split(".")[1]
        assert name.startswith("blocks.") and block in "01"
        files["winattn_layer_grads_block" + block]["grad." + name] = grad.numpy()
    for name, d in sorted(files.items()):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < 32 << 10, (name, os.path.getsize(path))
        print("wrote %s (%d bytes)" % (name, os.path.getsize(path)))


if __name__ == "__main__":
    main()
