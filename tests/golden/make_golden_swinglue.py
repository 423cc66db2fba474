"""Records tests/golden/swinglue_layer*.npz from the REFERENCE's own BasicLayer (src/models/swin_backbone.py) with
``downsample=PatchMerging``, in float64 on the CPU and in eval mode: dim 16, depth 2 (one block without a shift, one with a shift
of 2), 2 heads, window 4, mlp_ratio 2, every drop rate 0; input [2, 7 * 9, 16] with H = 7 and W = 9, so the window map pads to
8 x 12 and the patch merging pads both axes, to a 4 x 5 map.  Tensors only; each file under 32 KiB.

    python tests/golden/make_golden_swinglue.py /path/to/reference

The reference module is imported as make_golden_winattn.py imports it (its ``import_reference``).

``swinglue_layer`` holds the input ``x``, the state dict (``state.*``) and the gradients given on the two outputs, ``grad_out``
(on ``x_out``) and ``grad_down`` (on ``x_down``) -- values exact in float16, stored in float16; the index buffers as they are.
``swinglue_layer_out`` holds the float64 ``x_out`` and ``x_down``, ``swinglue_layer_grad_x`` the float64 ``grad.x``.  The float64
gradients of the parameters have files of their own: ``swinglue_layer_grads_block0``, ``swinglue_layer_grads_block1`` and ``swinglue_layer_grads_downsample``.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_winattn as base  # noqa: E402

LAYER = dict(dim=16, depth=2, num_heads=2, window_size=4, mlp_ratio=2.0)
B, H, W = 2, 7, 9


def main():
    if base.REFERENCE is None:
        raise SystemExit(__doc__)
    swin = base.import_reference()
    g = torch.Generator().manual_seed(2201)
    layer = swin.BasicLayer(qkv_bias=True, qk_scale=None, drop=0.0, attn_drop=0.0, drop_path=0.0, norm_layer=torch.nn.LayerNorm,
                            downsample=swin.PatchMerging, use_checkpoint=False, **LAYER).double().eval()
    assert [blk.shift_size for blk in layer.blocks] == [0, 2]
    base.fill(layer, g)
    x = base.exact16(B, H * W, LAYER["dim"], generator=g).requires_grad_(True)
    grad_out = base.exact16(B, H * W, LAYER["dim"], generator=g)
    grad_down = base.exact16(B, ((H + 1) // 2) * ((W + 1) // 2), 2 * LAYER["dim"], generator=g)
    x_out, h, w, x_down, h2, w2 = layer(x, H, W)
    assert (h, w, h2, w2) == (H, W, 4, 5) and x_down.shape == grad_down.shape
    params = dict(layer.named_parameters())
    grads = torch.autograd.grad([x_out, x_down], [x] + list(params.values()), [grad_out, grad_down])
    half = lambda t: t.detach().to(torch.float16).numpy()      # noqa: E731
    for t in [x, grad_out, grad_down] + list(params.values()):
        assert torch.equal(t.detach().to(torch.float16).double(), t.detach()), "not exact in float16"
    main_file = {"x": half(x), "grad_out": half(grad_out), "grad_down": half(grad_down)}
    for name, t in layer.state_dict().items():
        main_file["state." + name] = half(t) if t.is_floating_point() else t.numpy()
    files = {"swinglue_layer": main_file,
             "swinglue_layer_out": {"x_out": x_out.detach().numpy(), "x_down": x_down.detach().numpy()},
             "swinglue_layer_grad_x": {"grad.x": grads[0].numpy()},
             "swinglue_layer_grads_block0": {}, "swinglue_layer_grads_block1": {}, "swinglue_layer_grads_downsample": {}}
    for name, grad in zip(params, grads[1:]):
        part = "downsample" if name.startswith("downsample.") else "block" + name.split(".")[1]
        files["swinglue_layer_grads_" + part]["grad." + name] = grad.numpy()
    for name, d in sorted(files.items()):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < 32 << 10, (name, os.path.getsize(path))
        print("wrote %s (%d bytes)" % (name, os.path.getsize(path)))


if __name__ == "__main__":
    main()
