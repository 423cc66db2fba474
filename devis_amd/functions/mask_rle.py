"""Host side of the run-length encoder of the clip stitching (include/maskrle.h): from logit maps to
the COCO run lengths of the binarised full-resolution masks.  Argument checks, the output and workspace tensors and the two
kernel passes.  The custom op of :mod:`devis_amd.ops` runs exactly this code.

An inference operator like those of :mod:`devis_amd.functions.mask_iou`: no autograd formula, and an input that requires a
gradient while gradients are recorded raises.  The results are integers and depend on a mask's logits and the target size
alone.  Nothing of the target's resolution is allocated in bytes: the workspace holds one bit per pixel.

There is no CPU path and no eager fallback: CPU tensors raise, a failing kernel call raises.
"""
import torch

from .. import _maskrle, _native
from ._common import _check_device, _require
from .mask_iou import check_size

OP = "mask_run_lengths"


def default_max_runs(H, W):
    """The cap on a row's counts when the caller names none: 8 runs per column and one, or every pixel a run of its own where
    that is less.  (A compact region has at most two transitions per column, 2*W + 1 runs.)"""
    return min(H * W + 1, 8 * W + 1)


def check_max_runs(max_runs):
    if max_runs < 1:
        raise ValueError("%s: max_runs must be at least 1, got %r" % (OP, max_runs))
    return max_runs


def check_src(src, size, max_runs):
    """Shape and dtype contract of mask_run_lengths on [N, h, w] maps; raises before anything is launched.  Works on fake
    tensors.  Returns (N, h, w, H, W, max_runs)."""
    _require(src.dim() == 3, "%s: src must be [N, h, w]" % OP)
    _native.dtype_code(src.dtype)       # raises on an unsupported dtype
    H, W = check_size(OP, size)
    N, h, w = src.shape
    _require(h > 0 and w > 0, "%s: a map would be empty (%s x %s)" % (OP, h, w))
    _require(H * W <= 0x7fffffff, "%s: the target size %s x %s does not fit 31 bits" % (OP, H, W))
    return N, h, w, H, W, check_max_runs(max_runs)


def _run_lengths(src, size, max_runs):
    """int32 [N, 1 + max_runs]: per mask the number of runs, then its counts (include/maskrle.h)."""
    N, h, w, H, W, max_runs = check_src(src, size, max_runs)
    _check_device(OP, [("src", src)])
    runs = torch.empty((N, 1 + max_runs), dtype=torch.int32, device=src.device)
    if N:
        workspace = torch.empty(_maskrle.workspace_bytes(N, H, W), dtype=torch.uint8, device=src.device)
        _maskrle.encode(_native.dtype_code(src.dtype), src.contiguous(), N, h, w, H, W, max_runs, workspace, runs)
    return runs
