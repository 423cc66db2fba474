"""Records tests/golden/labelloss_*.npz from the REFERENCE's criterion, in float64 on the CPU: SetCriterion.loss_labels_focal
(src/models/criterion.py) with the reference's own sigmoid_focal_loss (src/models/deformable_segmentation.py) and accuracy
(src/util/misc.py) makes loss_ce, class_error and, by autograd, d loss_ce / d logits; the one-hot tensor it hands to
sigmoid_focal_loss -- captured there -- gives its target_classes.  Tensors only; a few kilobytes each.

    python tests/golden/make_golden_labelloss.py /path/to/reference

The reference modules are imported as make_golden_boxmatch.py imports them -- a package whose __init__ is skipped, with
stand-ins for what the criterion's imports pull in and never call here (pycocotools, visdom, the mask utilities, and
torchvision where it is missing).

Cases: a DeVIS clip of three frames with two targets, one target frame invalid; the same with a mask that is all False; two
images with 3 + 2 targets; and the inputs and the recorded matching of boxmatch_devis_mean.npz, the label loss as it runs
behind the matcher.

Every matched query's two largest logits are more than 1e-2 apart (the generator reseeds until they are), so the recorded
class_error cannot hinge on a tie.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else None
F64 = torch.float64
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
    for name in ("pycocotools", "pycocotools.mask", "visdom", "refsrc.util.mask_ops", "refsrc.models.ops", "refsrc.models.ops.modules"):
        sys.modules.setdefault(name, _Anything(name))
    try:
        import torchvision.ops.boxes  # noqa: F401
    except ImportError:
        boxes = types.ModuleType("torchvision.ops.boxes")
        boxes.box_area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        for name in ("torchvision", "torchvision.ops", "torchvision.ops.misc"):
            sys.modules[name] = _Anything(name)
        sys.modules["torchvision"].__version__ = "0.0"
        sys.modules["torchvision.ops.boxes"] = boxes
    criterion = importlib.import_module("refsrc.models.criterion")
    assert criterion.__file__ == os.path.join(src, "models", "criterion.py")
    assert criterion.sigmoid_focal_loss.__module__ == "refsrc.models.deformable_segmentation"
    assert criterion.accuracy.__module__ == "refsrc.util.misc"
    return criterion


class Recorder:
    """Takes sigmoid_focal_loss's place in the reference criterion's module: keeps the one-hot targets it is handed."""

    def __init__(self, real):
        self.real, self.onehot = real, []

    def __call__(self, inputs, targets, *a, **k):
        self.onehot.append(targets.detach().clone())
        return self.real(inputs, targets, *a, **k)


def run(criterion_mod, logits, targets, indices, num_boxes):
    """(loss_ce, class_error, target_classes, d loss_ce / d logits) of the reference's loss_labels_focal."""
    C = logits.shape[-1]
    crit = criterion_mod.SetCriterion(C, None, {}, 0.1, ["labels"], True, ALPHA)
    rec = Recorder(criterion_mod.sigmoid_focal_loss)
    criterion_mod.sigmoid_focal_loss = rec
    try:
        x = logits.clone().requires_grad_(True)
        out = crit.loss_labels_focal({"pred_logits": x}, targets, indices, num_boxes, log=True)
    finally:
        criterion_mod.sigmoid_focal_loss = rec.real
    grad, = torch.autograd.grad(out["loss_ce"], x)
    onehot, = rec.onehot
    assert tuple(onehot.shape) == tuple(logits.shape) and bool((onehot.sum(-1) <= 1).all())
    classes = torch.where(onehot.sum(-1) > 0, onehot.argmax(-1), torch.full(onehot.shape[:2], C))
    return {"loss_ce": out["loss_ce"].detach().numpy(), "class_error": torch.as_tensor(out["class_error"]).double().numpy(),
            "target_classes": classes.numpy().astype(np.int64), "grad_logits": grad.numpy()}


def top_two_margin(logits, rows):
    """The least lead of the largest logit over the runner-up among the (flattened) queries ``rows``."""
    if rows.numel() == 0:
        return float("inf")
    top = logits.reshape(-1, logits.shape[-1])[rows].topk(2, dim=1).values
    return float((top[:, 0] - top[:, 1]).min())


def devis_case(criterion_mod, seed, all_false):
    Fr, Q, C, T = 3, 7, 5, 2
    while True:
        g = torch.Generator().manual_seed(seed)
        logits = 2 * torch.randn(1, Fr * Q, C, generator=g, dtype=F64)
        labels = torch.randint(0, C, (T * Fr,), generator=g)
        out_i = torch.randperm(Q, generator=g)[:T]
        tgt_i = torch.randperm(T, generator=g)
        valid = torch.ones(T * Fr, dtype=torch.bool)
        if all_false:
            valid[:] = False
        else:
            valid[int(torch.randint(0, T * Fr, (1,), generator=g))] = False         # one target frame is invalid
        frames = torch.arange(Fr)
        index_i = (frames[None] * Q + out_i[:, None]).reshape(-1)       # as DeVISHungarianMatcher.forward forms them
        index_j = (frames[None] + tgt_i[:, None] * Fr).reshape(-1)
        index_valid = valid[index_j]
        for t in range(T):                                              # some matched queries are right, as in training
            if t % 2 == 0:
                for f in range(Fr):
                    logits[0, int(index_i[t * Fr + f]), int(labels[int(index_j[t * Fr + f])])] += 6.0
        if top_two_margin(logits, index_i) > MARGIN:
            break
        seed += 1000
    num_boxes = 2.0
    d = run(criterion_mod, logits, [{"labels": labels, "valid": valid}], [(index_i, index_j, index_valid)], num_boxes)
    d.update({"logits": logits.numpy(), "labels": labels.numpy(), "valid": valid.numpy(), "index_i": index_i.numpy(),
              "index_j": index_j.numpy(), "index_valid": index_valid.numpy(), "dims": np.array([Fr, Q, C, T], dtype=np.int64),
              "num_boxes": np.array(num_boxes), "margin": np.array(top_two_margin(logits, index_i))})
    return d


def image_case(criterion_mod, seed):
    B, Q, C, sizes = 2, 7, 5, (3, 2)
    while True:
        g = torch.Generator().manual_seed(seed)
        logits = 2 * torch.randn(B, Q, C, generator=g, dtype=F64)
        targets = [{"labels": torch.randint(0, C, (n,), generator=g)} for n in sizes]
        indices = [(torch.randperm(Q, generator=g)[:n].sort().values, torch.randperm(n, generator=g)) for n in sizes]
        for b, (i, j) in enumerate(indices):
            logits[b, int(i[0]), int(targets[b]["labels"][int(j[0])])] += 6.0
        rows = torch.cat([b * Q + i for b, (i, _) in enumerate(indices)])
        if top_two_margin(logits, rows) > MARGIN:
            break
        seed += 1000
    num_boxes = 5.0
    d = run(criterion_mod, logits, targets, indices, num_boxes)
    d.update({"logits": logits.numpy(), "dims": np.array([B, Q, C], dtype=np.int64), "sizes": np.array(sizes, dtype=np.int64),
              "num_boxes": np.array(num_boxes), "margin": np.array(top_two_margin(logits, rows))})
    for b, (t, (i, j)) in enumerate(zip(targets, indices)):
        d.update({"labels_%d" % b: t["labels"].numpy(), "index_i_%d" % b: i.numpy(), "index_j_%d" % b: j.numpy()})
    return d


def matched_case(criterion_mod):
    """The inputs and the recorded matching of boxmatch_devis_mean.npz (four targets; made by the reference's matcher): what
    the label loss sees behind the matcher."""
    src = np.load(os.path.join(HERE, "boxmatch_devis_mean.npz"))
    logits, labels, valid = (torch.from_numpy(src[k]) for k in ("logits", "labels", "valid"))
    index_i, index_j, index_valid = (torch.from_numpy(src[k]) for k in ("index_i", "index_j", "index_valid"))
    assert top_two_margin(logits, index_i) > MARGIN
    num_boxes = 4.0
    d = run(criterion_mod, logits, [{"labels": labels, "valid": valid}], [(index_i, index_j, index_valid)], num_boxes)
    d.update({"logits": logits.numpy(), "labels": labels.numpy(), "valid": valid.numpy(), "index_i": index_i.numpy(),
              "index_j": index_j.numpy(), "index_valid": index_valid.numpy(), "dims": src["dims"],
              "num_boxes": np.array(num_boxes), "margin": np.array(top_two_margin(logits, index_i))})
    return d


def main():
    if REFERENCE is None:
        raise SystemExit(__doc__)
    criterion_mod = import_reference()
    cases = {"labelloss_devis": devis_case(criterion_mod, 4100, False), "labelloss_devis_none": devis_case(criterion_mod, 4200, True),
             "labelloss_image": image_case(criterion_mod, 4300), "labelloss_devis_matched": matched_case(criterion_mod)}
    for name, d in sorted(cases.items()):
        d["alpha"] = np.array(ALPHA)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < 32 << 10
        print("wrote %s (%d bytes), loss_ce %.6f, class_error %.3f, margin %.3f"
              % (name, os.path.getsize(path), float(d["loss_ce"]), float(d["class_error"]), float(d["margin"])))


if __name__ == "__main__":
    main()
