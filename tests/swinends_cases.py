"""What the tests of the Swin backbone's ends share (tests/ only): a ``PatchEmbed`` and a ``SwinTransformer`` with the attribute
names, parameter names and call signatures of the reference's ``src/models/swin_backbone.py``, written anew, on top of
tests/swinglue_cases.py's ``BasicLayer`` and ``PatchMerging``.  This module stands in for ``src.models.swin_backbone`` in
``devis_amd.patch_swin_ends(swinends_cases)`` -- and in ``patch_swin_glue`` and ``patch_window_attention``, whose classes it
re-exports.  The fixture tests/golden/swinends_*.npz was recorded from the reference's own ``SwinTransformer``
(tests/golden/make_golden_swinends.py)."""
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

import swinglue_cases as SG
from swinglue_cases import BasicLayer, PatchMerging, SwinTransformerBlock  # noqa: F401  (the stage's classes, by the reference's names)

GOLDEN = SG.GOLDEN
BACKBONE = dict(embed_dim=8, depths=[1, 1], num_heads=[1, 2], window_size=2, patch_size=4, mlp_ratio=2.0, out_indices=(0, 1))
IMAGE = (2, 3, 10, 13)                  # both axes are padded: 3 x 4 tokens, merged (with padding) to 2 x 2
FILES = ("swinends_backbone", "swinends_backbone_out", "swinends_backbone_grads_ends", "swinends_backbone_grads_layer0",
         "swinends_backbone_grads_layer1")


class PatchEmbed(nn.Module):
    def __init__(self, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        self.patch_size = (patch_size, patch_size) if isinstance(patch_size, int) else tuple(patch_size)
        self.in_chans, self.embed_dim = in_chans, embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.patch_size)
        self.norm = norm_layer(embed_dim) if norm_layer is not None else None

    def forward(self, x):
        H, W = x.shape[2:]
        ph, pw = self.patch_size
        if W % pw:
            x = F.pad(x, (0, pw - W % pw))
        if H % ph:
            x = F.pad(x, (0, 0, 0, ph - H % ph))
        x = self.proj(x)
        if self.norm is not None:
            Wh, Ww = x.shape[2:]
            x = self.norm(x.flatten(2).transpose(1, 2))
            x = x.transpose(1, 2).view(-1, self.embed_dim, Wh, Ww)
        return x


class SwinTransformer(nn.Module):
    def __init__(self, pretrain_img_size=224, patch_size=4, in_chans=3, embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24),
                 window_size=7, mlp_ratio=4.0, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0, norm_layer=nn.LayerNorm,
                 ape=False, patch_norm=True, out_indices=(0, 1, 2, 3), use_checkpoint=False):
        super().__init__()
        self.num_layers, self.embed_dim, self.ape, self.patch_norm, self.out_indices = len(depths), embed_dim, ape, patch_norm, out_indices
        self.patch_embed = PatchEmbed(patch_size, in_chans, embed_dim, norm_layer if patch_norm else None)
        if ape:
            size = pretrain_img_size // patch_size
            self.absolute_pos_embed = nn.Parameter(torch.zeros(1, embed_dim, size, size))
        self.pos_drop = nn.Dropout(p=drop_rate)
        rates = torch.linspace(0, drop_path_rate, sum(depths)).tolist()
        self.layers = nn.ModuleList([
            BasicLayer(embed_dim * 2 ** i, depths[i], num_heads[i], window_size, mlp_ratio, attn_drop=attn_drop_rate,
                       drop_path=rates[sum(depths[:i]):sum(depths[:i + 1])], norm_layer=norm_layer,
                       downsample=PatchMerging if i < len(depths) - 1 else None, use_checkpoint=use_checkpoint)
            for i in range(len(depths))])
        self.num_features = [embed_dim * 2 ** i for i in range(len(depths))]
        for i in out_indices:
            self.add_module("norm%d" % i, norm_layer(self.num_features[i]))

    def forward(self, x):
        x = self.patch_embed(x)
        Wh, Ww = x.shape[2:]
        if self.ape:
            x = x + F.interpolate(self.absolute_pos_embed, size=(Wh, Ww), mode="bicubic")
        x = self.pos_drop(x.flatten(2).transpose(1, 2))
        outs = []
        for i, layer in enumerate(self.layers):
            x_out, H, W, x, Wh, Ww = layer(x, Wh, Ww)
            if i in self.out_indices:
                x_out = getattr(self, "norm%d" % i)(x_out)
                outs.append(x_out.view(-1, H, W, self.num_features[i]).permute(0, 3, 1, 2).contiguous())
        return {str(u): v for u, v in enumerate(outs)}


# ---- the fixture -------------------------------------------------------------------------------------------------------------

def load_fixture():
    """{name: float64 tensor} of tests/golden/swinends_backbone.npz and its result files."""
    case = {}
    for name in FILES:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
            case.update({k: torch.from_numpy(f[k].astype(np.float64) if f[k].dtype.kind == "f" else f[k]) for k in f.files})
    return case


def build_backbone(case=None, dtype=torch.float64, device="cpu", **kwargs):
    """The recorded backbone -- with the fixture's state dict when ``case`` is given -- in eval mode, and its image."""
    model = SwinTransformer(**dict(BACKBONE, **kwargs)).to(dtype)
    if case is not None:
        state = {k[len("state."):]: v for k, v in case.items() if k.startswith("state.")}
        assert sorted(state) == sorted(model.state_dict())
        model.load_state_dict(state)
        image = case["image"]
    else:
        image = torch.randn(*IMAGE, generator=torch.Generator().manual_seed(78))
    return model.to(device).eval(), image.to(device=device, dtype=dtype)


def run_backbone(model, image, case):
    """{"out.0", "out.1", "grad.<parameter>"} of one forward and backward with the fixture's gradients on the two outputs."""
    outs = model(image)
    assert sorted(outs) == ["0", "1"]
    params = dict(model.named_parameters())
    to = lambda t: t.to(device=image.device, dtype=outs["0"].dtype)      # noqa: E731
    grads = torch.autograd.grad([outs["0"], outs["1"]], list(params.values()), [to(case["grad_out.0"]), to(case["grad_out.1"])])
    got = {"out.0": outs["0"].detach(), "out.1": outs["1"].detach()}
    got.update({"grad." + name: g for name, g in zip(params, grads)})
    return got


def expected(case):
    """The recorded results: the two outputs and the gradient of every parameter."""
    return {k: v for k, v in case.items() if k.startswith("out.") or k.startswith("grad.")}
