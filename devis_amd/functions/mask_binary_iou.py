"""Host side of the binary mask IoU of the clip stitching (include/maskbiou.h): from two sets of logit
maps to the pixel counts of the binarised full-resolution masks -- per pair and frame the intersection, per map its area --
and to the IoU matrix made of them.  Argument checks, the output and workspace tensors and the kernel passes.  The custom
ops of :mod:`devis_amd.ops` run exactly this code.

An inference operator like those of :mod:`devis_amd.functions.mask_iou`: no autograd formula, and an input that requires a
gradient while gradients are recorded raises.  The counts are integers and depend on a pair's logits and the target size
alone.  Nothing of the target's resolution is allocated in bytes: the workspace holds one bit per pixel.

There is no CPU path and no eager fallback: CPU tensors raise, a failing kernel call raises.
"""
import torch

from .. import _maskbiou, _native
from ._common import _check_device, _require
from .mask_iou import check_size

OP = "mask_binary_iou"
REDUCE = ("volume", "frame")


def check_reduce(reduce):
    if reduce not in REDUCE:
        raise ValueError("%s: reduce must be 'volume' or 'frame', got %r" % (OP, reduce))
    return reduce


def check_pair(a, b, size):
    """Shape and dtype contract of mask_binary_iou on [N, F, h, w] maps; raises before anything is launched.  Works on fake
    tensors.  Returns (Na, Nb, F, h, w, H, W)."""
    _require(a.dim() == 4 and b.dim() == 4, "%s: a and b must be [N, F, h, w]" % OP)
    _native.dtype_code(a.dtype)       # raises on an unsupported dtype
    _require(a.dtype == b.dtype, "%s: a is %s, b is %s" % (OP, a.dtype, b.dtype))
    H, W = check_size(OP, size)
    Na, F, h, w = a.shape
    Nb = b.shape[0]
    _require(tuple(b.shape[1:]) == (F, h, w), "%s: b has maps of %s, a of %s" % (OP, tuple(b.shape[1:]), (F, h, w)))
    _require(F > 0 and h > 0 and w > 0, "%s: a map would be empty (%s frames of %s x %s)" % (OP, F, h, w))
    _require(H * W <= 0x7fffffff, "%s: the target size %s x %s does not fit 31 bits" % (OP, H, W))
    return Na, Nb, F, h, w, H, W


def _terms(a, b, size):
    """(inter [Na, Nb, F], area_a [Na, F], area_b [Nb, F]) int32 (include/maskbiou.h).  a, b [N, F, h, w]."""
    Na, Nb, F, h, w, H, W = check_pair(a, b, size)
    _check_device(OP, [("a", a), ("b", b)])
    new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=a.device)      # noqa: E731
    inter, area_a, area_b = new(Na, Nb, F), new(Na, F), new(Nb, F)
    if Na == 0 and Nb == 0:
        return inter, area_a, area_b
    if Na == 0 or Nb == 0:
        # the areas of the side that has maps: a call of that side against its own first map (an area depends on its map alone)
        maps = b if Na == 0 else a
        areas = _terms(maps, maps[:1], size)[1]
        return (inter, area_a, areas) if Na == 0 else (inter, areas, area_b)
    workspace = torch.empty(_maskbiou.workspace_bytes(Na, Nb, F, H, W), dtype=torch.uint8, device=a.device)
    _maskbiou.counts(_native.dtype_code(a.dtype), a.contiguous(), b.contiguous(), Na, Nb, F, h, w, H, W, workspace, inter,
                     area_a, area_b)
    return inter, area_a, area_b


def ratio(inter, area_a, area_b, reduce):
    """float64 [Na, Nb] from the counts, formed in int64 where the tensors are: "volume" sums the frames' intersections and
    unions and divides once; "frame" divides per frame and takes the mean.  A ratio whose union is 0 is 0.0."""
    inter, area_a, area_b = inter.long(), area_a.long(), area_b.long()
    if reduce == "volume":
        inter, area_a, area_b = inter.sum(2, keepdim=True), area_a.sum(1, keepdim=True), area_b.sum(1, keepdim=True)
    union = area_a[:, None, :] + area_b[None, :, :] - inter
    iou = inter.double() / union.clamp(min=1).double()           # (a union of 0 has an intersection of 0)
    total = iou[:, :, 0]
    for f in range(1, iou.shape[2]):            # the frames in ascending order, then one division: numpy's mean(axis=0)
        total = total + iou[:, :, f]
    # (by a tensor: a division by a Python number is a multiplication by its rounded reciprocal on the device)
    return total / torch.full_like(total, iou.shape[2])


def _binary_iou(a, b, size, reduce):
    """float64 [Na, Nb]: :func:`ratio` of :func:`_terms`."""
    check_reduce(reduce)
    return ratio(*_terms(a, b, size), reduce)
