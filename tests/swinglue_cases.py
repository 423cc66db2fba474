"""What the Swin-glue tests share (tests/ only): a reference-shaped stage -- tests/winattn_cases.py's ``Mlp``, ``WindowAttention``
and ``SwinTransformerBlock`` as they are, a ``BasicLayer`` with the reference's ``drop_path`` and ``downsample`` arguments, and a
``DropPath`` and a ``PatchMerging`` with the attribute names, parameter names and call signatures of the reference's
``src/models/swin_backbone.py`` and of ``timm.models.layers.DropPath`` (``timm`` is not a dependency), written anew.  This module
stands in for ``src.models.swin_backbone`` in ``devis_amd.patch_swin_glue(swinglue_cases)`` and
``devis_amd.patch_window_attention(swinglue_cases)``.  The fixture tests/golden/swinglue_*.npz was recorded from the
reference's own ``BasicLayer`` with ``downsample=PatchMerging`` (tests/golden/make_golden_swinglue.py)."""
import os

import numpy as np
import torch
import torch.nn.functional as F
import torch.utils.checkpoint as checkpoint
from torch import nn

import winattn_cases as WC
import winattn_oracle as WO
from winattn_cases import Mlp, WindowAttention  # noqa: F401  (the stage's classes, by the reference's names)

GOLDEN = WC.GOLDEN
LAYER = dict(dim=16, depth=2, num_heads=2, window_size=4, mlp_ratio=2.0)        # the recorded stage
LAYER_INPUT = (2, 7, 9)                 # B, H, W: the window map pads to 8 x 12, the merge pads both axes to 4 x 5
FILES = ("swinglue_layer", "swinglue_layer_out", "swinglue_layer_grad_x", "swinglue_layer_grads_block0", "swinglue_layer_grads_block1",
         "swinglue_layer_grads_downsample")


class DropPath(nn.Module):
    """Stochastic depth per sample (``timm.models.layers.DropPath``): in training a sample is zeroed with probability
    ``drop_prob`` and the others are scaled by ``1 / keep_prob``."""

    def __init__(self, drop_prob=0.0, scale_by_keep=True):
        super().__init__()
        self.drop_prob, self.scale_by_keep = drop_prob, scale_by_keep

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep_prob = 1 - self.drop_prob
        random_tensor = x.new_empty((x.shape[0],) + (1,) * (x.ndim - 1)).bernoulli_(keep_prob)
        if keep_prob > 0.0 and self.scale_by_keep:
            random_tensor.div_(keep_prob)
        return x * random_tensor


class SwinTransformerBlock(WC.SwinTransformerBlock):
    """The stand-in block of tests/winattn_cases.py with the reference's ``drop_path`` argument."""

    def __init__(self, dim, num_heads, window_size=7, shift_size=0, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop=0.0,
                 attn_drop=0.0, drop_path=0.0):
        super().__init__(dim, num_heads, window_size, shift_size, mlp_ratio, qkv_bias, qk_scale, drop, attn_drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()

    forward = WC.SwinTransformerBlock.forward               # (a function of this class: a patch of it leaves winattn_cases' alone)


class PatchMerging(nn.Module):
    def __init__(self, dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = norm_layer(4 * dim)

    def forward(self, x, H, W):
        B, L, C = x.shape
        assert L == H * W
        x = x.view(B, H, W, C)
        if H % 2 == 1 or W % 2 == 1:
            x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
        x = torch.cat([x[:, 0::2, 0::2, :], x[:, 1::2, 0::2, :], x[:, 0::2, 1::2, :], x[:, 1::2, 1::2, :]], -1)
        return self.reduction(self.norm(x.view(B, -1, 4 * C)))


class BasicLayer(nn.Module):
    built_masks = 0                     # how often a forward built the shift mask (the tests count it)

    def __init__(self, dim, depth, num_heads, window_size=7, mlp_ratio=4.0, attn_drop=0.0, drop_path=0.0, norm_layer=nn.LayerNorm,
                 downsample=None, use_checkpoint=False):
        super().__init__()
        self.window_size, self.shift_size, self.depth, self.use_checkpoint = window_size, window_size // 2, depth, use_checkpoint
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim, num_heads, window_size, 0 if i % 2 == 0 else window_size // 2, mlp_ratio, attn_drop=attn_drop,
                                 drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path) for i in range(depth)])
        self.downsample = downsample(dim=dim, norm_layer=norm_layer) if downsample is not None else None

    def forward(self, x, H, W):
        ws = self.window_size
        Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
        type(self).built_masks += 1
        attn_mask = WO.sliced_mask(Hp, Wp, ws, self.shift_size).to(device=x.device, dtype=x.dtype)
        for blk in self.blocks:
            blk.H, blk.W = H, W
            x = checkpoint.checkpoint(blk, x, attn_mask, use_reentrant=False) if self.use_checkpoint else blk(x, attn_mask)
        if self.downsample is not None:
            return x, H, W, self.downsample(x, H, W), (H + 1) // 2, (W + 1) // 2
        return x, H, W, x, H, W


# ---- the fixture -------------------------------------------------------------------------------------------------------------

def load_fixture():
    """{name: float64 tensor} of tests/golden/swinglue_layer.npz and its result files."""
    case = {}
    for name in FILES:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
            case.update({k: torch.from_numpy(f[k].astype(np.float64) if f[k].dtype.kind == "f" else f[k]) for k in f.files})
    return case


def build_layer(case=None, dtype=torch.float64, device="cpu", **kwargs):
    """The recorded stage -- with the fixture's state dict when ``case`` is given -- in eval mode, and its input (a leaf)."""
    layer = BasicLayer(**LAYER, downsample=PatchMerging, **kwargs).to(dtype)
    if case is not None:
        state = {k[len("state."):]: v for k, v in case.items() if k.startswith("state.")}
        assert sorted(state) == sorted(layer.state_dict())
        layer.load_state_dict(state)
        x = case["x"]
    else:
        B, H, W = LAYER_INPUT
        x = torch.randn(B, H * W, LAYER["dim"], generator=torch.Generator().manual_seed(77))
    layer = layer.to(device).eval()
    return layer, x.to(device=device, dtype=dtype).requires_grad_(True)


def run_layer(layer, x, case):
    """{"x_out", "x_down", "grad.x", "grad.<parameter>"} of one forward and backward of the recorded stage, with the fixture's
    ``grad_out`` and ``grad_down`` on the two outputs."""
    B, H, W = LAYER_INPUT
    result = layer(x, H, W)
    x_out, x_down = result[0], result[3]
    assert tuple(result[1:3]) == (H, W) and tuple(result[4:]) == ((H + 1) // 2, (W + 1) // 2)
    params = dict(layer.named_parameters())
    to = lambda t: t.to(device=x_out.device, dtype=x_out.dtype)      # noqa: E731
    grads = torch.autograd.grad([x_out, x_down], [x] + list(params.values()), [to(case["grad_out"]), to(case["grad_down"])])
    got = {"x_out": x_out.detach(), "x_down": x_down.detach(), "grad.x": grads[0]}
    got.update({"grad." + name: g for name, g in zip(params, grads[1:])})
    return got
