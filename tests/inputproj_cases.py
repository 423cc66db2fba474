"""What the CPU and the GPU tests of the input projections share (include/inputproj.h): the shapes, the
cases with their oracle results, and a stand-in for the reference's model around the projections -- a ``DeformableDETR``-shaped
module with an ``input_proj`` ``ModuleList`` and a ``DeformableTransformer``-shaped one with ``prepare_data``, written anew with
the reference's attribute names -- which loads the fixture tests/golden/inputproj_model.npz
(tests/golden/make_golden_inputproj.py).

This module doubles as the "reference module" the patches take: ``devis_amd.patch_transformer(inputproj_cases)`` and
``devis_amd.patch_position_encoding(inputproj_cases, inputproj_cases)`` find the classes they patch here by name.
"""
import functools
import os

import numpy as np
import torch
from torch import nn

import inputproj_oracle as O

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
PYRAMID = ((5, 7), (3, 4), (2, 2), (1, 1))
# ((C, G), levels, what it covers): the table of the issue, and `means` x `batches` of each
SHAPES = [
    ((256, 32), PYRAMID, "the configuration, with an 8-element group"),
    ((256, 32), ((3, 5), (2, 3), (1, 2), (1, 1)), "small maps"),
    ((8, 4), PYRAMID[:3], "few channels"),
    ((6, 6), ((5, 7), (3, 4), (2, 4)), "one channel per group, per-element stores"),
    ((12, 4), PYRAMID, "odd channels per group"),
    ((40, 8), PYRAMID, "five channels per group"),
    ((260, 4), PYRAMID, "channel-tile tail"),
    ((1024, 32), ((2, 3), (1, 1)), "the limit"),
    ((8, 1), PYRAMID, "one group"),
    ((256, 32), ((17, 23),), "3128 elements per group: most of one statistics chunk (4096)"),
    ((256, 32), ((9, 130),), "pixel-tile tails; three statistics chunks and three chunks of the backward's sums"),
    # added: the statistics chunk is 4096 elements, so 17 x 23 stays in one; the smallest map of 8-channel groups that spans two
    ((256, 32), ((19, 27),), "4104 elements per group: two statistics chunks, the second of 8 elements; two chunks of the sums"),
]
MEANS = (0.0, 4.0)
BATCHES = (1, 3)
# (maps, parameters, tokens)
MIXES = [(BF16, BF16, BF16), (F16, F16, F16), (BF16, F32, F32), (F16, F32, F32), (F32, F32, BF16), (F32, F32, F16)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputproj_model.npz")


def min_group(C, G, levels):
    return min(C // G * h * w for h, w in levels)


def oracle_checks(shape):
    """The checks of one row of ``SHAPES`` as (N, C, G, levels, mean, gradients): every mean and batch; a row with a level whose
    groups have fewer than 4 elements -- (12, 4) on 1 x 1 -- is a forward check as it stands and a gradient check without that
    level (tests/test_inputproj_gpu.py says why)."""
    (C, G), levels, _ = shape
    kept = tuple(hw for hw in levels if C // G * hw[0] * hw[1] >= 4)
    for mean in MEANS:
        for N in BATCHES:
            yield N, C, G, levels, mean, kept == levels
            if kept and kept != levels:
                yield N, C, G, kept, mean, True


def rand(*shape, seed, dtype=F32, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) + shift).to(dtype)


@functools.lru_cache(maxsize=None)
def case(N, C, G, levels, mean=0.0, mix=(F32, F32, F32)):
    """(inputs on the CPU, rounded to their storage dtypes; the oracle's results).  The inputs and results are shared by the
    tests: nobody writes to them."""
    xdt, pdt, ydt = mix
    d = {"xs": [rand(N, C, h, w, seed=100 + l, dtype=xdt, shift=mean) for l, (h, w) in enumerate(levels)],
         "weights": [rand(C, seed=200 + l, dtype=pdt, shift=1.0) for l in range(len(levels))],
         "biases": [rand(C, seed=300 + l, dtype=pdt) for l in range(len(levels))],
         "grad_tokens": rand(N, sum(h * w for h, w in levels), C, seed=400, dtype=ydt), "num_groups": G}
    want = O.forward(d["xs"], G, d["weights"], d["biases"])
    want.update(O.grads(d["xs"], G, d["weights"], d["grad_tokens"]))
    return d, want


def run(d, fn, out_dtype=None, wants=None, device=None):
    """{tokens, grad_x, grad_weight, grad_bias} of ``fn`` (the operator or its composite) on the case's tensors, moved to
    ``device`` when given; ``wants`` = three lists of bools (default: everything)."""
    L = len(d["xs"])
    wants = wants or ([True] * L,) * 3
    move = (lambda t: t.to(device)) if device is not None else (lambda t: t)
    leaves = [[move(t).detach().requires_grad_(w) for t, w in zip(d[k], ws)] for k, ws in zip(("xs", "weights", "biases"), wants)]
    tokens = fn(leaves[0], d["num_groups"], leaves[1], leaves[2], out_dtype=out_dtype)
    flat = [t for group in leaves for t in group]
    asked = [t for t in flat if t.requires_grad]
    grads = iter(torch.autograd.grad(tokens, asked, move(d["grad_tokens"])) if asked else ())
    each = [next(grads) if t.requires_grad else None for t in flat]
    return {"tokens": tokens.detach(), "grad_x": each[:L], "grad_weight": each[L:2 * L], "grad_bias": each[2 * L:]}


def deviation(got, want):
    """max|got - want| / max|want|, the quantity of the project's bars."""
    want = want.double()
    return float((got.detach().double().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-300)


# ---- the stand-in model ------------------------------------------------------------------------------------------------------

class NestedTensor:
    def __init__(self, tensors, mask):
        self.tensors, self.mask = tensors, mask

    def decompose(self):
        return self.tensors, self.mask


class PositionEmbeddingSine(nn.Module):
    """The reference's constructor arguments and attributes; the stand-in's forward is all zeros (the patches replace it)."""

    def __init__(self, num_pos_feats=64, temperature=10000, normalize=False, scale=None):
        super().__init__()
        self.num_pos_feats, self.temperature, self.normalize, self.scale = num_pos_feats, temperature, normalize, scale or 6.283185307179586

    def forward(self, tensor_list):
        m = tensor_list.mask
        return torch.zeros(m.shape[0], 2 * self.num_pos_feats, *m.shape[1:], device=m.device)


class PositionEmbeddingSineWithLearnableTemporal(PositionEmbeddingSine):
    pass


class DeformableTransformerEncoder(nn.Module):
    @staticmethod
    def get_reference_points(spatial_shapes, valid_ratios, device):
        raise NotImplementedError


class DeformableTransformer(nn.Module):
    """``prepare_data`` as the reference states it, and a forward that returns it with the shapes read off ``srcs``."""

    def __init__(self, d_model, num_feature_levels):
        super().__init__()
        self.d_model = d_model
        self.level_embed = nn.Parameter(torch.zeros(num_feature_levels, d_model))

    def get_valid_ratio(self, mask):
        _, H, W = mask.shape
        return torch.stack([torch.sum(~mask[:, 0, :], 1).float() / W, torch.sum(~mask[:, :, 0], 1).float() / H], -1)

    def prepare_data(self, srcs, masks, pos_embeds):
        flat, pads, embeds, shapes = [], [], [], []
        for lvl, (src, mask, pos) in enumerate(zip(srcs, masks, pos_embeds)):
            shapes.append(tuple(src.shape[2:]))
            flat.append(src.flatten(2).transpose(1, 2))
            pads.append(mask.flatten(1))
            embeds.append(pos.flatten(2).transpose(1, 2) + self.level_embed[lvl].view(1, 1, -1))
        flat, pads, embeds = torch.cat(flat, 1), torch.cat(pads, 1), torch.cat(embeds, 1)
        spatial = torch.as_tensor(shapes, dtype=torch.long, device=flat.device)
        starts = torch.cat((spatial.new_zeros((1,)), spatial.prod(1).cumsum(0)[:-1]))
        return flat, pads, embeds, spatial, starts, torch.stack([self.get_valid_ratio(m) for m in masks], 1)

    def forward(self, srcs, masks, pos_embeds):
        out = self.prepare_data(srcs, masks, pos_embeds)
        return out, [tuple(src.shape) for src in srcs]


class DeformableDETR(nn.Module):
    """``input_proj`` as the reference constructs it for ``num_feature_levels`` levels over the backbone's channels: 1 x 1
    projections, then 3 x 3 / stride-2 ones, each followed by ``GroupNorm(32, hidden_dim)``; and the part of its forward that
    builds ``srcs``, ``masks`` and ``pos`` and calls the transformer."""

    def __init__(self, num_channels, hidden_dim, num_feature_levels):
        super().__init__()
        self.num_feature_levels = num_feature_levels
        layers, in_channels = [], None
        for in_channels in num_channels:
            layers.append(nn.Sequential(nn.Conv2d(in_channels, hidden_dim, kernel_size=1), nn.GroupNorm(32, hidden_dim)))
        for _ in range(num_feature_levels - len(num_channels)):
            layers.append(nn.Sequential(nn.Conv2d(in_channels, hidden_dim, kernel_size=3, stride=2, padding=1), nn.GroupNorm(32, hidden_dim)))
            in_channels = hidden_dim
        self.input_proj = nn.ModuleList(layers)
        self.position = PositionEmbeddingSineWithLearnableTemporal(hidden_dim // 2, normalize=True)
        self.transformer = DeformableTransformer(hidden_dim, num_feature_levels)

    def forward(self, features):
        srcs, masks, pos = [], [], []
        for l, feat in enumerate(features):
            src = self.input_proj[l](feat)
            mask = torch.zeros(feat.shape[0], *feat.shape[2:], dtype=torch.bool, device=feat.device)
            srcs.append(src)
            masks.append(mask)
            pos.append(self.position(NestedTensor(src, mask)).to(src.dtype))
        for l in range(len(features), self.num_feature_levels):
            src = self.input_proj[l](features[-1] if l == len(features) else srcs[-1])
            mask = torch.zeros(src.shape[0], *src.shape[-2:], dtype=torch.bool, device=features[-1].device)
            pos.append(self.position(NestedTensor(src, mask)).to(src.dtype))
            srcs.append(src)
            masks.append(mask)
        (src_flatten, *_), shapes = self.transformer(srcs, masks, pos)
        return src_flatten, srcs, shapes


@functools.lru_cache(maxsize=None)
def load_fixture():
    with np.load(GOLDEN) as f:
        return {k: torch.from_numpy(f[k]) for k in f.files}


def build_model(fixture, dtype, device):
    """(model, features): the stand-in with the fixture's state dict, and the fixture's features as leaves."""
    state = {k[6:]: v.to(dtype) for k, v in fixture.items() if k.startswith("state.")}
    channels = [fixture["feature.%d" % l].shape[1] for l in range(3)]
    model = DeformableDETR(channels, state["0.1.weight"].shape[0], 4).to(device=device, dtype=dtype)
    model.input_proj.load_state_dict(state)
    features = [fixture["feature.%d" % l].to(device=device, dtype=dtype).requires_grad_(True) for l in range(3)]
    return model, features


def run_model(model, features, fixture):
    """{src_flatten, grad.<name>, grad_feature.<l>} of the stand-in, by the fixture's loss: through the encoder input and through
    a consumer of ``srcs[1]``; and (srcs, src_flatten) as the model returned them."""
    src_flatten, srcs, shapes = model(features)
    assert shapes == [tuple(s.shape) for s in srcs]
    params = dict(model.input_proj.named_parameters())
    consumer = srcs[1] * 1.0                                                            # (what the mask head does: arithmetic on srcs[l])
    loss = (src_flatten.double() * fixture["grad_tokens"].to(src_flatten.device).double()).sum() + \
        (consumer.double() * fixture["grad_src1"].to(consumer.device).double()).sum()
    grads = torch.autograd.grad(loss, list(params.values()) + list(features))
    got = {"src_flatten": src_flatten.detach()}
    got.update({"grad." + name: g for name, g in zip(params, grads)})
    got.update({"grad_feature.%d" % l: g for l, g in enumerate(grads[len(params):])})
    return got, srcs, src_flatten


def expected(fixture):
    return {k: v for k, v in fixture.items() if k == "src_flatten" or k.startswith("grad.") or k.startswith("grad_feature.")}
