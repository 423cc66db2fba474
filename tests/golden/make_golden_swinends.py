"""Records tests/golden/swinends_backbone*.npz from the REFERENCE's own SwinTransformer (src/models/swin_backbone.py), in float64
on the CPU and in eval mode: embed_dim 8, depths [1, 1], heads [1, 2], window 2, patch 4, mlp_ratio 2, out_indices (0, 1), patch
norm, no absolute position embedding, every drop rate 0; image [2, 3, 10, 13], so the patch embedding pads both axes (3 x 4
tokens) and so does the patch merging (2 x 2).  Tensors only; each file under 32 KiB.

    python tests/golden/make_golden_swinends.py /path/to/reference

The reference module is imported as make_golden_winattn.py imports it (its ``import_reference``).

``swinends_backbone`` holds the ``image``, the state dict (``state.*``) and the gradients given on the two outputs,
``grad_out.0`` and ``grad_out.1`` -- values exact in float16, stored in float16; the index buffers as they are.
``swinends_backbone_out`` holds the float64 outputs ``out.0`` and ``out.1``.  The float64 gradients ``grad.<name>`` of the
parameters have files of their own: ``swinends_backbone_grads_ends`` (the patch embedding and the output norms),
``swinends_backbone_grads_layer0`` and ``swinends_backbone_grads_layer1``.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_winattn as base  # noqa: E402

BACKBONE = dict(embed_dim=8, depths=[1, 1], num_heads=[1, 2], window_size=2, patch_size=4, mlp_ratio=2.0, out_indices=(0, 1))
IMAGE = (2, 3, 10, 13)


def main():
    if base.REFERENCE is None:
        raise SystemExit(__doc__)
    swin = base.import_reference()
    g = torch.Generator().manual_seed(2401)
    model = swin.SwinTransformer(drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0, ape=False, patch_norm=True,
                                 frozen_stages=-1, use_checkpoint=False, **BACKBONE).double()
    model.eval()                                            # (the reference's train() returns nothing)
    base.fill(model, g)
    with torch.no_grad():                                   # (fill() knows the blocks' norms by ".norm": the four others)
        for name, p in model.named_parameters():
            if name.startswith("norm") and name.endswith("weight"):
                p.copy_((p + 1.0).to(torch.float16).double())
    image = base.exact16(*IMAGE, generator=g)
    outs = model(image)
    assert sorted(outs) == ["0", "1"] and outs["0"].shape == (2, 8, 3, 4) and outs["1"].shape == (2, 16, 2, 2)
    grad_outs = [base.exact16(*outs[k].shape, generator=g) for k in ("0", "1")]
    params = dict(model.named_parameters())
    grads = torch.autograd.grad([outs["0"], outs["1"]], list(params.values()), grad_outs)
    half = lambda t: t.detach().to(torch.float16).numpy()      # noqa: E731
    for t in [image] + grad_outs + list(params.values()):
        assert torch.equal(t.detach().to(torch.float16).double(), t.detach()), "not exact in float16"
    main_file = {"image": half(image), "grad_out.0": half(grad_outs[0]), "grad_out.1": half(grad_outs[1])}
    for name, t in model.state_dict().items():
        main_file["state." + name] = half(t) if t.is_floating_point() else t.numpy()
    files = {"swinends_backbone": main_file,
             "swinends_backbone_out": {"out." + k: outs[k].detach().numpy() for k in ("0", "1")},
             "swinends_backbone_grads_ends": {}, "swinends_backbone_grads_layer0": {}, "swinends_backbone_grads_layer1": {}}
    for name, grad in zip(params, grads):
        part = "layer" + name.split(".")[1] if name.startswith("layers.") else "ends"
        files["swinends_backbone_grads_" + part]["grad." + name] = grad.numpy()
    for name, d in sorted(files.items()):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < 32 << 10, (name, os.path.getsize(path))
        print("wrote %s (%d bytes)" % (name, os.path.getsize(path)))


if __name__ == "__main__":
    main()
