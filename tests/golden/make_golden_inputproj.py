"""Records tests/golden/inputproj_model.npz from the REFERENCE, in float64 on the CPU: the ``input_proj`` list as
``DeformableDETR.__init__`` (src/models/deformable_detr.py) constructs it, and ``DeformableTransformer.prepare_data``
(src/models/deformable_transformer.py).  Tensors only; the file stays under 96 KiB.

    python tests/golden/make_golden_inputproj.py /path/to/reference

The reference's modules are imported as make_golden_posembed.py imports them (its ``import_reference``).  The whole
``DeformableDETR.forward`` needs a backbone and the transformer's CUDA extension, so the fixture is recorded from the two pieces
that can be run here:

* ``DeformableDETR(backbone, transformer, ...)`` is constructed with stand-ins that carry only what the constructor reads
  (``backbone.num_channels`` / ``strides``, ``transformer.d_model`` / ``decoder``); its ``input_proj`` is the reference's own
  construction: hidden_dim 64, so ``GroupNorm(32, 64)`` has groups of 2 channels; three 1 x 1 levels on 4, 6 and 8 channels
  and one 3 x 3 / stride-2 level on the last feature map.  The projections are applied by the rule of ``forward``
  (deformable_detr.py:153-170): level ``l < 3`` to feature ``l``, level 3 to the last feature.
* ``DeformableTransformer.prepare_data`` is called unbound on a stand-in that has the level embedding, with all-False masks and
  zero position embeddings; its first result is ``src_flatten``.

Features are [2, C_l, H_l, W_l] on 5 x 7, 3 x 4 and 2 x 2 (the fourth level is 1 x 1).  The gradients are those of
``sum(src_flatten * grad_tokens) + sum(srcs[1] * grad_src1)``: through the encoder input and through a consumer of ``srcs[1]``.
``grad_tokens`` is 0 on the fourth level's token: its groups have 2 elements, where the gradient of a GroupNorm is a
cancellation that float32 does not resolve (the forward of that level is in the fixture).

``feature.<l>``, ``state.<name>`` (the state dict of ``input_proj``), ``grad_tokens`` and ``grad_src1`` hold values exact in
float16, stored in float16; ``src_flatten``, ``grad.<name>`` (parameters) and ``grad_feature.<l>`` are the float64 results
rounded once to float32 (6e-8 of a value, against bars of 1e-4), which halves the file.
"""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_posembed as base  # noqa: E402

HIDDEN, CHANNELS, SIZES, FRAMES = 64, (4, 6, 8), ((5, 7), (3, 4), (2, 2)), 2


def exact16(*shape, generator, shift=0.0):
    return (torch.randn(*shape, generator=generator) + shift).to(torch.float16).double()


def main():
    if base.REFERENCE is None:
        raise SystemExit(__doc__)
    import importlib
    _, transformer = base.import_reference()
    detr = importlib.import_module("refsrc.models.deformable_detr")
    backbone = nn.Module()
    backbone.num_channels, backbone.strides = [4] + list(CHANNELS), [4, 8, 16, 32]
    top = nn.Module()
    top.d_model, top.decoder = HIDDEN, nn.Module()
    top.decoder.num_layers = 1
    model = detr.DeformableDETR(backbone, top, num_classes=2, num_queries=3, num_feature_levels=4, aux_loss=False,
                                with_box_refine=False, with_ref_point_refine=False, with_gradient=False)
    proj = model.input_proj.double()
    assert len(proj) == 4 and [p[0].kernel_size for p in proj] == [(1, 1)] * 3 + [(3, 3)] and proj[3][0].stride == (2, 2)
    g = torch.Generator().manual_seed(2501)
    with torch.no_grad():
        for name, p in proj.named_parameters():
            norm_weight = name.endswith("1.weight")
            scale = 0.25 if p.dim() > 1 else 1.0
            p.copy_((exact16(*p.shape, generator=g, shift=1.0 if norm_weight else 0.0) * scale).to(torch.float16).double())
    features = [exact16(FRAMES, c, h, w, generator=g, shift=0.5 * l).requires_grad_(True)
                for l, (c, (h, w)) in enumerate(zip(CHANNELS, SIZES))]
    srcs = [proj[l](features[l]) for l in range(3)]
    srcs.append(proj[3](features[-1]))
    assert tuple(srcs[3].shape) == (FRAMES, HIDDEN, 1, 1)
    stand_in = types.SimpleNamespace(level_embed=torch.zeros(4, HIDDEN, dtype=torch.float64))
    stand_in.get_valid_ratio = types.MethodType(transformer.DeformableTransformer.get_valid_ratio, stand_in)
    masks = [torch.zeros(FRAMES, *s.shape[2:], dtype=torch.bool) for s in srcs]
    pos = [torch.zeros_like(s) for s in srcs]
    src_flatten = transformer.DeformableTransformer.prepare_data(stand_in, srcs, masks, pos)[0]
    tokens = sum(h * w for h, w in SIZES) + 1
    assert tuple(src_flatten.shape) == (FRAMES, tokens, HIDDEN)
    grad_tokens = exact16(FRAMES, tokens, HIDDEN, generator=g)
    grad_tokens[:, -1] = 0.0
    grad_src1 = exact16(*srcs[1].shape, generator=g)
    params = dict(proj.named_parameters())
    loss = (src_flatten * grad_tokens).sum() + (srcs[1] * grad_src1).sum()
    grads = torch.autograd.grad(loss, list(params.values()) + features)
    half = lambda t: t.detach().to(torch.float16).numpy()      # noqa: E731
    single = lambda t: t.detach().to(torch.float32).numpy()    # noqa: E731
    d = {"src_flatten": single(src_flatten), "grad_tokens": half(grad_tokens), "grad_src1": half(grad_src1)}
    for l, f in enumerate(features):
        d["feature.%d" % l] = half(f)
        d["grad_feature.%d" % l] = single(grads[len(params) + l])
    for name, t in proj.state_dict().items():
        assert torch.equal(t.to(torch.float16).double(), t), name
        d["state." + name] = half(t)
    for name, grad in zip(params, grads):
        d["grad." + name] = single(grad)
    path = os.path.join(HERE, "inputproj_model.npz")
    np.savez_compressed(path, **d)
    assert os.path.getsize(path) < 96 << 10, os.path.getsize(path)
    print("wrote inputproj_model (%d bytes)" % os.path.getsize(path))


if __name__ == "__main__":
    main()
