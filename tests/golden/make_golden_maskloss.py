"""Records tests/golden/maskloss_*.npz from the REFERENCE's own sigmoid_focal_loss and dice_loss
(src/models/deformable_segmentation.py), composed as SetCriterion.loss_masks composes them -- with
F.interpolate(..., mode="bilinear", align_corners=False), which is what the reference's interpolate wrapper calls -- in
float64 on the CPU: the logits, the bool targets, num_boxes, alpha, both losses and the gradient of their sum with respect
to the logits.  Tensors only; a few kilobytes each.

    python tests/golden/make_golden_maskloss.py [/path/to/reference]

The reference module is imported as make_golden_attmap.py imports it.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from make_golden_attmap import import_reference_segmentation

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = {   # name -> (N, (h, w), (H, W), alpha, num_boxes, special targets)
    "maskloss_up": (3, (7, 9), (27, 35), 0.25, 3.0, ()),
    "maskloss_video": (4, (12, 20), (45, 80), 0.25, 2.5, ("empty", "full")),
    "maskloss_down": (2, (26, 22), (13, 11), 0.25, 2.0, ()),
    "maskloss_noalpha": (3, (9, 7), (20, 33), -1.0, 4.0, ()),
}


def blobs(g, N, H, W):
    """Bool masks with structure: a thresholded smooth random field per instance."""
    coarse = torch.randn(N, 1, max(H // 6, 2), max(W // 6, 2), generator=g, dtype=torch.float64)
    return F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=False)[:, 0] > 0.1


def main():
    seg = import_reference_segmentation()
    for seed, (name, (N, (h, w), (H, W), alpha, num_boxes, special)) in enumerate(sorted(CASES.items())):
        g = torch.Generator().manual_seed(3000 + seed)
        src = (2.5 * torch.randn(N, h, w, generator=g, dtype=torch.float64)).requires_grad_(True)
        target = blobs(g, N, H, W)
        for i, kind in enumerate(special):
            target[1 + i] = kind == "full"
        t = target.to(src).flatten(1)
        x = F.interpolate(src[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0].flatten(1)
        loss_mask = seg.sigmoid_focal_loss(x, t, num_boxes, alpha=alpha)
        loss_dice = seg.dice_loss(x, t, num_boxes)
        grad, = torch.autograd.grad(loss_mask + loss_dice, src)
        d = {"src": src.detach(), "target": target, "num_boxes": torch.tensor(num_boxes, dtype=torch.float64),
             "alpha": torch.tensor(alpha, dtype=torch.float64), "loss_mask": loss_mask.detach(),
             "loss_dice": loss_dice.detach(), "grad_src": grad}
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **{k: v.numpy() for k, v in d.items()})
        print("wrote %s: %s" % (name, {k: tuple(v.shape) for k, v in d.items()}))


if __name__ == "__main__":
    main()
