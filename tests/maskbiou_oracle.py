"""Oracle of the binary mask IoU (include/maskbiou.h), in numpy and plain torch on the CPU: the counts from the bits of
tests/maskiou_oracle.py (imported, not copied), the two ratios in float64, and the reference's pairwise ``iou`` written out
on boolean arrays -- its truthiness branches and its frames without a detection.  No reference code in it."""
import numpy as np
import torch

import maskiou_oracle as O


def counts_of_bits(A, B):
    """(inter [Na, Nb, F], area_a [Na, F], area_b [Nb, F]) int64 from bool arrays A [Na, F, ...] and B [Nb, F, ...]."""
    A = np.asarray(A).reshape(A.shape[0], A.shape[1], -1).astype(np.int64)
    B = np.asarray(B).reshape(B.shape[0], B.shape[1], -1).astype(np.int64)
    return np.einsum("ifk,jfk->ijf", A, B), A.sum(2), B.sum(2)


def bits(src, size, arith=torch.float32):
    """bool numpy [N, F, H, W] of src [N, F, h, w], by ``maskiou_oracle.binarize``."""
    N, F = src.shape[:2]
    return O.binarize(src.flatten(0, 1), size, arith)[0].reshape(N, F, size[0], size[1]).numpy()


def counts(a, b, size, arith=torch.float32):
    """The counts of a [Na, F, h, w] and b [Nb, F, h, w] at ``size``."""
    return counts_of_bits(bits(a, size, arith), bits(b, size, arith))


def iou(inter, area_a, area_b, reduce):
    """float64 [Na, Nb] from integer counts: "volume" divides the sums over the frames once, "frame" divides per frame and
    takes the mean (the frames added in ascending order, then one division); 0.0 where a union is 0."""
    inter, area_a, area_b = (np.asarray(t).astype(np.int64) for t in (inter, area_a, area_b))
    if reduce == "volume":
        inter, area_a, area_b = inter.sum(2, keepdims=True), area_a.sum(1, keepdims=True), area_b.sum(1, keepdims=True)
    union = area_a[:, None, :] + area_b[None, :, :] - inter
    ratio = np.where(union > 0, inter.astype(np.float64) / np.maximum(union, 1).astype(np.float64), 0.0)
    total = np.zeros(ratio.shape[:2])
    for f in range(ratio.shape[2]):
        total = total + ratio[:, :, f]
    return total / ratio.shape[2]


def reference_iou(track1_masks, track2_masks):
    """The reference's ``HungarianInferenceMatcher.iou`` of two tracks' windows, written out: a frame is a bool array or
    None; a pair of frames with both masks adds their intersection and union, with one mask that mask's area to the union."""
    i, u = 0.0, 0.0
    for d, g in zip(track1_masks, track2_masks):
        if d is not None and g is not None:
            i += int(np.logical_and(d, g).sum())
            u += int(np.logical_or(d, g).sum())
        elif d is None and g is not None:
            u += int(g.sum())
        elif d is not None and g is None:
            u += int(d.sum())
    return i / u if u > 0.0 else 0.0


def reference_volume(windows1, windows2):
    """[len(windows1), len(windows2)] of :func:`reference_iou`."""
    return np.array([[reference_iou(d, g) for g in windows2] for d in windows1], dtype=np.float64).reshape(len(windows1), len(windows2))


def reference_frame(windows1, windows2):
    """The frame-average cost: per frame the IoU matrix of the frame's masks (0.0 for a pair without a set pixel), stacked
    and averaged over the frames."""
    frames = len(windows1[0])
    per = [reference_volume([[d[t]] for d in windows1], [[g[t]] for g in windows2]) for t in range(frames)]
    return np.stack(per, axis=0).mean(axis=0)
