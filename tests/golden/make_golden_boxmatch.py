"""Records tests/golden/boxmatch_*.npz from the REFERENCE's criterion, in float64 on the CPU: DeVISHungarianMatcher.forward and
HungarianMatcher.forward (src/models/matcher.py) make the cost matrices -- captured where they are handed to
linear_sum_assignment -- and the index tensors; F.l1_loss and box_ops.generalized_box_iou (src/util/box_ops.py), composed as
SetCriterion.loss_boxes composes them, make the box losses and their gradient.  Tensors only; a few kilobytes each.

    python tests/golden/make_golden_boxmatch.py [/path/to/reference]

The reference modules are imported as make_golden_maskiou.py imports them -- a package whose __init__ is skipped, with
pycocotools and the mask utilities as stand-ins -- except that src/util/box_ops.py is the real file.  It imports
torchvision.ops.boxes.box_area: where torchvision is missing, a one-line stand-in takes its place.

Every assignment problem is checked, by brute force over all assignments, to have an optimum that beats the runner-up by more
than 1e-2 in total cost (the generator reseeds until it does), so the recorded indices cannot hinge on rounding.
"""
import importlib
import itertools
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
F64 = torch.float64
WEIGHTS = dict(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)
ALPHA = 0.25
MARGIN = 1e-2


class _Anything(types.ModuleType):
    """A stand-in module: any attribute is a placeholder class (enough for `from x import Y`)."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def import_reference():
    src = os.path.join(REFERENCE, "src")
    for name, path in (("refsrc", src), ("refsrc.models", os.path.join(src, "models")), ("refsrc.util", os.path.join(src, "util"))):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    for name in ("pycocotools", "pycocotools.mask", "refsrc.util.mask_ops"):
        sys.modules.setdefault(name, _Anything(name))
    try:
        import torchvision.ops.boxes  # noqa: F401
    except ImportError:
        boxes = types.ModuleType("torchvision.ops.boxes")
        boxes.box_area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        for name in ("torchvision", "torchvision.ops"):
            sys.modules[name] = _Anything(name)
        sys.modules["torchvision.ops.boxes"] = boxes
    box_ops = importlib.import_module("refsrc.util.box_ops")
    assert box_ops.__file__ == os.path.join(src, "util", "box_ops.py")
    return importlib.import_module("refsrc.models.matcher"), box_ops


def random_boxes(g, *shape):
    """cxcywh boxes inside the unit square with sides of 0.1 .. 0.5."""
    wh = 0.1 + 0.4 * torch.rand(*shape, 2, generator=g, dtype=F64)
    centre = 0.25 + 0.5 * torch.rand(*shape, 2, generator=g, dtype=F64)
    return torch.cat([centre, wh], -1)


def margin(cost):
    """The optimum's lead over the runner-up among all assignments of the columns of ``cost`` [R, T] to distinct rows."""
    R, T = cost.shape
    cols = np.arange(T)
    totals = sorted(float(cost[list(rows), cols].sum()) for rows in itertools.permutations(range(R), T))
    return totals[1] - totals[0] if len(totals) > 1 else float("inf")


class Recorder:
    """Takes linear_sum_assignment's place in the reference matcher's module: keeps what it is handed."""

    def __init__(self, solve):
        self.solve, self.costs = solve, []

    def __call__(self, cost):
        self.costs.append(torch.as_tensor(cost).numpy().astype(np.float64))
        return self.solve(cost)


def devis_case(matcher_mod, use_sum, seed):
    Fr, Q, C, T = 3, 7, 5, 4
    while True:
        g = torch.Generator().manual_seed(seed)
        logits = 2 * torch.randn(1, Fr * Q, C, generator=g, dtype=F64)
        boxes = random_boxes(g, 1, Fr * Q)
        labels = torch.randint(0, C, (T * Fr,), generator=g)
        tgt_boxes = random_boxes(g, T * Fr)
        valid = torch.rand(T * Fr, generator=g) > 0.3
        matcher = matcher_mod.DeVISHungarianMatcher(num_frames=Fr, num_queries=Q, focal_loss=True, focal_alpha=ALPHA,
                                                    use_l1_distance_sum=use_sum, **WEIGHTS)
        rec = Recorder(matcher_mod.linear_sum_assignment)
        matcher_mod.linear_sum_assignment = rec
        try:
            (index_i, index_j, index_valid), = matcher({"pred_logits": logits, "pred_boxes": boxes},
                                                       [{"labels": labels, "boxes": tgt_boxes, "valid": valid}])
        finally:
            matcher_mod.linear_sum_assignment = rec.solve
        cost, = rec.costs
        assert cost.shape == (Q, T)
        if margin(cost) > MARGIN:
            break
        seed += 1000
    assert index_i.dtype == index_j.dtype == torch.int64 and index_valid.dtype == torch.bool
    return {"logits": logits.numpy(), "boxes": boxes.numpy(), "labels": labels.numpy(), "tgt_boxes": tgt_boxes.numpy(),
            "valid": valid.numpy(), "cost": cost, "index_i": index_i.numpy(), "index_j": index_j.numpy(),
            "index_valid": index_valid.numpy(), "dims": np.array([Fr, Q, C, T], dtype=np.int64), "use_sum": np.array(use_sum),
            "margin": np.array(margin(cost))}


def image_case(matcher_mod, seed):
    B, Q, C, sizes = 2, 7, 5, (3, 2)
    while True:
        g = torch.Generator().manual_seed(seed)
        logits = 2 * torch.randn(B, Q, C, generator=g, dtype=F64)
        boxes = random_boxes(g, B, Q)
        targets = [{"labels": torch.randint(0, C, (n,), generator=g), "boxes": random_boxes(g, n)} for n in sizes]
        matcher = matcher_mod.HungarianMatcher(focal_loss=True, focal_alpha=ALPHA, **WEIGHTS)
        rec = Recorder(matcher_mod.linear_sum_assignment)
        matcher_mod.linear_sum_assignment = rec
        try:
            indices = matcher({"pred_logits": logits, "pred_boxes": boxes}, targets)
        finally:
            matcher_mod.linear_sum_assignment = rec.solve
        assert [c.shape for c in rec.costs] == [(Q, n) for n in sizes]
        if min(margin(c) for c in rec.costs) > MARGIN:
            break
        seed += 1000
    d = {"logits": logits.numpy(), "boxes": boxes.numpy(), "dims": np.array([B, Q, C], dtype=np.int64),
         "sizes": np.array(sizes, dtype=np.int64), "margin": np.array(min(margin(c) for c in rec.costs))}
    for b, (t, c, (i, j)) in enumerate(zip(targets, rec.costs, indices)):
        assert i.dtype == j.dtype == torch.int64
        d.update({"labels_%d" % b: t["labels"].numpy(), "tgt_boxes_%d" % b: t["boxes"].numpy(), "cost_%d" % b: c,
                  "index_i_%d" % b: i.numpy(), "index_j_%d" % b: j.numpy()})
    return d


def boxes_case(box_ops, seed):
    N, num_boxes = 9, 4.0
    g = torch.Generator().manual_seed(seed)
    src, target = random_boxes(g, N), random_boxes(g, N)
    src[0] = target[0]                                                                   # every tie at once
    src[1], target[1] = torch.tensor([0.2, 0.2, 0.2, 0.1], dtype=F64), torch.tensor([0.7, 0.8, 0.3, 0.2], dtype=F64)    # disjoint
    src[2], target[2] = torch.tensor([0.5, 0.5, 0.2, 0.1], dtype=F64), torch.tensor([0.45, 0.55, 0.6, 0.5], dtype=F64)  # nested
    src.requires_grad_(True)
    loss_bbox = F.l1_loss(src, target, reduction="none").sum() / num_boxes
    loss_giou = (1 - torch.diag(box_ops.generalized_box_iou(box_ops.box_cxcywh_to_xyxy(src),
                                                            box_ops.box_cxcywh_to_xyxy(target)))).sum() / num_boxes
    grad, = torch.autograd.grad(loss_bbox + loss_giou, src)
    return {"src": src.detach().numpy(), "target": target.numpy(), "num_boxes": np.array(num_boxes),
            "loss_bbox": loss_bbox.detach().numpy(), "loss_giou": loss_giou.detach().numpy(), "grad_src": grad.numpy()}


def main():
    matcher_mod, box_ops = import_reference()
    cases = {"boxmatch_devis_mean": devis_case(matcher_mod, False, 3100), "boxmatch_devis_sum": devis_case(matcher_mod, True, 3200),
             "boxmatch_image": image_case(matcher_mod, 3300), "boxmatch_boxes": boxes_case(box_ops, 3400)}
    for name, d in sorted(cases.items()):
        d.update({k: np.array(v) for k, v in WEIGHTS.items()}, alpha=np.array(ALPHA))
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < 32 << 10
        print("wrote %s (%d bytes)%s" % (name, os.path.getsize(path), ", margin %.3f" % float(d["margin"]) if "margin" in d else ""))


if __name__ == "__main__":
    main()
