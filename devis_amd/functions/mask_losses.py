"""Host side of the mask loss (include/maskloss.h): bilinear resampling of the logit maps to the
target resolution, sigmoid focal loss and dice loss as one operator that returns the two per-instance vectors.  Argument
checks, the output and workspace tensors, and the kernel passes of forward and backward.  The custom ops of
:mod:`devis_amd.ops` run exactly this code.

Every sum has a fixed order -- there are no float atomics -- so the losses and grad_src are bitwise reproducible and nothing
here raises or warns under ``torch.use_deterministic_algorithms(True)``.  Nothing of the target's resolution is allocated.

There is no CPU path and no eager fallback: CPU tensors raise, a failing kernel call raises.
"""
import math

import torch

from .. import _maskloss, _native
from ._common import _check_device, _require, eager_backward


def check_gamma(gamma):
    """The exponents the kernels apply: 0, 1 and anything larger than 1 (2 is a square, the others ``pow``).  0 < gamma < 1
    has an unbounded derivative where p_t is 1, a negative one is no focal loss: both raise ValueError."""
    gamma = float(gamma)
    if not (gamma == 0.0 or (gamma >= 1.0 and math.isfinite(gamma))):
        raise ValueError("mask_loss_terms: gamma must be 0, 1 or larger than 1, got %r" % (gamma,))
    return gamma


def check_shapes(src, target):
    """Shape and dtype contract of mask_loss_terms; raises before anything is launched.  Works on fake tensors.  Returns
    (N, h, w, H, W, the target kind of include/maskloss.h)."""
    _require(src.dim() == 3, "mask_loss_terms: src_masks must be [N, h, w] (or [N, 1, h, w])")
    _require(target.dim() == 3, "mask_loss_terms: target_masks must be [N, H, W]")
    _native.dtype_code(src.dtype)       # raises on an unsupported dtype
    kind = _maskloss.target_kind(src.dtype, target.dtype)
    N, h, w = src.shape
    _require(target.shape[0] == N, "mask_loss_terms: target_masks has %s instances, src_masks %s" % (target.shape[0], N))
    H, W = target.shape[1], target.shape[2]
    _require(h > 0 and w > 0 and H > 0 and W > 0, "mask_loss_terms: a map would be empty (%s x %s -> %s x %s)" % (h, w, H, W))
    return N, h, w, H, W, kind


def _forward(src, target, alpha, gamma):
    """(focal [N], dice [N], sums [N, 3]) in the arithmetic type: float32, float64 for float64 logits."""
    N, h, w, H, W, kind = check_shapes(src, target)
    gamma = check_gamma(gamma)
    _check_device("mask_loss_terms", [("src_masks", src), ("target_masks", target)])
    acc = _native.acc_dtype(src.dtype)
    focal, dice = torch.empty((N,), dtype=acc, device=src.device), torch.empty((N,), dtype=acc, device=src.device)
    sums = torch.empty((N, 3), dtype=acc, device=src.device)
    if N == 0:
        return focal, dice, sums
    shape = _maskloss.Shape(N, h, w, H, W)
    code = _native.dtype_code(src.dtype)
    nbytes = _maskloss.workspace_bytes(code, shape)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=src.device) if nbytes else None
    _maskloss.forward(code, kind, src.contiguous(), target.contiguous(), shape, alpha, gamma, workspace, focal, dice, sums)
    return focal, dice, sums


def _backward(grad_focal, grad_dice, src, target, sums, alpha, gamma):
    """grad_src [N, h, w] in src's dtype."""
    N, h, w, H, W, kind = check_shapes(src, target)
    gamma = check_gamma(gamma)
    _check_device("mask_loss_terms", [("src_masks", src), ("target_masks", target), ("sums", sums), ("grad_focal", grad_focal),
                   ("grad_dice", grad_dice)])
    acc = _native.acc_dtype(src.dtype)
    _require(tuple(sums.shape) == (N, 3) and sums.dtype == acc, "mask_loss_terms: sums must be [N, 3] in the arithmetic type")
    _require(tuple(grad_focal.shape) == (N,) and tuple(grad_dice.shape) == (N,), "mask_loss_terms: the gradients must be [N]")
    grad_src = torch.empty((N, h, w), dtype=src.dtype, device=src.device)
    if N == 0:
        return grad_src
    _maskloss.backward(_native.dtype_code(src.dtype), kind, src.contiguous(), target.contiguous(), sums.contiguous(),
                       grad_focal.to(acc).contiguous(), grad_dice.to(acc).contiguous(), _maskloss.Shape(N, h, w, H, W),
                       alpha, gamma, grad_src)
    return grad_src


def setup_context(ctx, inputs, output):
    src, target, alpha, gamma = inputs
    ctx.alpha, ctx.gamma = alpha, gamma
    ctx.mark_non_differentiable(output[2])
    ctx.save_for_backward(src, target, output[2])


def backward(run, ctx, grad_focal, grad_dice, grad_sums):
    """The autograd formula; ``run`` is :func:`_backward` or the backward op."""
    if not ctx.needs_input_grad[0]:
        return None, None, None, None
    src, target, sums = ctx.saved_tensors
    return run(grad_focal, grad_dice, src, target, sums, ctx.alpha, ctx.gamma), None, None, None


class MaskLossTermsFunction(torch.autograd.Function):
    """``mask_loss_terms`` for eager code: ``apply(src [N, h, w], target [N, H, W], alpha, gamma)`` -> (focal, dice, sums), the
    last without a gradient: the formula's ``setup_context`` reads it from the output, as the op's does.  Saves src, target as
    it was given and the [N, 3] sums.  No backward launch when src needs no gradient."""
    forward = staticmethod(_forward)
    setup_context = staticmethod(setup_context)
    backward = eager_backward(backward, _backward)
