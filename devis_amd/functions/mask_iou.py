"""Host side of the clip-stitching operators (include/maskiou.h): the soft mask IoU matrix between two
sets of logit maps and the binarised full-resolution masks.  Argument checks, the output and workspace tensors and the
kernel passes.  The custom ops of :mod:`devis_amd.ops` run exactly this code.

These are inference operators: there is no autograd formula, and an input that requires a gradient while gradients are
recorded raises.  Every sum has a fixed order -- there are no float atomics -- so the results are bitwise reproducible.
Nothing of the target's resolution is allocated in a floating type.

There is no CPU path and no eager fallback: CPU tensors raise, a failing kernel call raises.
"""
import torch

from .. import _maskiou, _native
from ._common import _check_device, _require, _workspace

REDUCE = {"volume": _maskiou.VOLUME, "frame": _maskiou.FRAME}
ORDER = {"C": _maskiou.ROW_MAJOR, "F": _maskiou.COL_MAJOR}


def check_reduce(reduce):
    if reduce not in REDUCE:
        raise ValueError("mask_soft_iou: reduce must be 'volume' or 'frame', got %r" % (reduce,))
    return reduce


def check_order(order):
    if order not in ORDER:
        raise ValueError("binarize_masks: order must be 'C' or 'F', got %r" % (order,))
    return order


def check_eps(eps):
    eps = float(eps)
    if not 0.0 <= eps < float("inf"):
        raise ValueError("mask_soft_iou: eps must be a finite number that is not negative, got %r" % (eps,))
    return eps


def check_size(op, size):
    _require(len(size) == 2, "%s: size must be (H, W), got %s" % (op, tuple(size)))
    H, W = size
    _require(H > 0 and W > 0, "%s: the target size %s x %s is empty" % (op, H, W))
    return H, W


def check_no_grad(op, named):
    """Inference operators: no input may ask for a gradient while gradients are recorded."""
    if torch.is_grad_enabled():
        for name, t in named:
            _require(not t.requires_grad, "%s: %s requires a gradient, and %s is an inference operator without a backward "
                     "(call it under torch.no_grad() or detach the input)" % (op, name, op))


def check_pair(a, b, size):
    """Shape and dtype contract of mask_soft_iou on [N, F, h, w] maps; raises before anything is launched.  Works on fake
    tensors.  Returns (Na, Nb, F, h, w, H, W)."""
    _require(a.dim() == 4 and b.dim() == 4, "mask_soft_iou: a and b must be [N, F, h, w] (or [N, h, w])")
    _native.dtype_code(a.dtype)       # raises on an unsupported dtype
    _require(a.dtype == b.dtype, "mask_soft_iou: a is %s, b is %s" % (a.dtype, b.dtype))
    H, W = check_size("mask_soft_iou", size)
    Na, F, h, w = a.shape
    Nb = b.shape[0]
    _require(tuple(b.shape[1:]) == (F, h, w), "mask_soft_iou: b has maps of %s, a of %s" % (tuple(b.shape[1:]), (F, h, w)))
    _require(F > 0 and h > 0 and w > 0, "mask_soft_iou: a map would be empty (%s frames of %s x %s)" % (F, h, w))
    return Na, Nb, F, h, w, H, W


def check_src(src, size):
    """The contract of binarize_masks; returns (N, h, w, H, W)."""
    _require(src.dim() == 3, "binarize_masks: src must be [N, h, w]")
    _native.dtype_code(src.dtype)
    H, W = check_size("binarize_masks", size)
    N, h, w = src.shape
    _require(h > 0 and w > 0, "binarize_masks: a map would be empty (%s x %s)" % (h, w))
    return N, h, w, H, W


def _pairwise(a, b, size, reduce, eps):
    """(iou [Na, Nb], inter [F, Na, Nb], sum_a [F, Na], sum_b [F, Nb]) in the arithmetic type: float32, float64 for float64
    logits.  a, b [N, F, h, w]."""
    Na, Nb, F, h, w, H, W = check_pair(a, b, size)
    check_reduce(reduce)
    eps = check_eps(eps)
    _check_device("mask_soft_iou", [("a", a), ("b", b)])
    acc = _native.acc_dtype(a.dtype)
    new = lambda *shape: torch.empty(shape, dtype=acc, device=a.device)      # noqa: E731
    iou, inter, sum_a, sum_b = new(Na, Nb), new(F, Na, Nb), new(F, Na), new(F, Nb)
    if Na == 0 and Nb == 0:
        return iou, inter, sum_a, sum_b
    if Na == 0 or Nb == 0:
        # the sums of the side that has maps: a call of that side against its own first map (a sum depends on its map alone)
        maps = b if Na == 0 else a
        sums = _pairwise(maps, maps[:1], size, reduce, eps)[2]
        return (iou, inter, sum_a, sums) if Na == 0 else (iou, inter, sums, sum_b)
    code = _native.dtype_code(a.dtype)
    shape = _maskiou.Shape(Na, Nb, F, h, w, H, W)
    workspace = _workspace(_maskiou, code, shape, a.device)
    _maskiou.pairwise(code, REDUCE[reduce], a.contiguous(), b.contiguous(), shape, eps, workspace, inter, sum_a, sum_b, iou)
    return iou, inter, sum_a, sum_b


def _binarize(src, size, order):
    """bool [N, H, W]: dense for ``order`` "C", the transposed view of a dense [N, W, H] for "F"."""
    N, h, w, H, W = check_src(src, size)
    check_order(order)
    _check_device("binarize_masks", [("src", src)])
    out = torch.empty((N, W, H) if order == "F" else (N, H, W), dtype=torch.bool, device=src.device)
    if N:
        _maskiou.binarize(_native.dtype_code(src.dtype), ORDER[order], src.contiguous(), N, h, w, H, W, out)
    return out.transpose(1, 2) if order == "F" else out
