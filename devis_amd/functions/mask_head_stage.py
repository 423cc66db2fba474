"""Host side of one stage of the mask head's glue (include/mhstage.h): GroupNorm, ReLU, nearest
upsampling, the FPN add and the concatenation of the attention maps as one operator whose result is channels-last.
Argument checks, the output, statistics and workspace tensors, and the kernel passes of forward and backward.  The custom
ops of :mod:`devis_amd.ops` run exactly this code.

Every sum has a fixed order -- there are no float atomics -- so ``out`` and all five gradients are bitwise reproducible and
nothing here raises or warns under ``torch.use_deterministic_algorithms(True)``.

There is no CPU path and no eager fallback: CPU tensors raise, a failing kernel call raises.
"""
import torch

from .. import _mhstage, _native
from ._common import _check_device, _require, _workspace, eager_backward

NEED_X, NEED_WEIGHT, NEED_BIAS, NEED_SKIP = _mhstage.GRAD_X, _mhstage.GRAD_WEIGHT, _mhstage.GRAD_BIAS, _mhstage.GRAD_SKIP
NEED_EXTRA = 16         # host only: a slice of grad_out
NEED_ALL = NEED_X | NEED_WEIGHT | NEED_BIAS | NEED_SKIP | NEED_EXTRA


def grads_mask(need_x, need_weight, need_bias, need_skip, need_extra):
    """``ctx.needs_input_grad`` flags -> the `grads` mask of the backward op."""
    return ((NEED_X if need_x else 0) | (NEED_WEIGHT if need_weight else 0) | (NEED_BIAS if need_bias else 0)
            | (NEED_SKIP if need_skip else 0) | (NEED_EXTRA if need_extra else 0))


def check_shapes(x, num_groups, weight, bias, skip=None, skip_index=None, extra=None, out_dtype=None):
    """Shape and dtype contract of mask_head_stage; raises before anything is launched.  Works on fake tensors.  Returns
    (N, F, C, G, E, h, w, H, W, out's dtype); F is 0 without a skip."""
    _require(x.dim() == 4, "mask_head_stage: x must be [N, C, h, w]")
    N, C, h, w = x.shape
    _require(isinstance(num_groups, int) and num_groups > 0, "mask_head_stage: num_groups must be a positive int")
    _require(C > 0 and C % num_groups == 0, "mask_head_stage: %s channels are not a multiple of the %d groups" % (C, num_groups))
    _require(h > 0 and w > 0, "mask_head_stage: the map would be empty (%s x %s)" % (h, w))
    _native.dtype_code(x.dtype)         # raises on an unsupported dtype
    _require(weight.dim() == 1 and weight.shape[0] == C and bias.dim() == 1 and bias.shape[0] == C,
             "mask_head_stage: weight and bias must be [C] = [%s]" % C)
    _mhstage.wide_dtype(x.dtype, weight.dtype, "weight")
    _require(bias.dtype == weight.dtype, "mask_head_stage: bias must have weight's dtype")
    F, E, size = 0, 0, None
    if skip is not None:
        _require(skip.dim() == 4 and skip.shape[1] == C, "mask_head_stage: skip must be [F, C, H, W] = [F, %s, H, W], got %s"
                 % (C, tuple(skip.shape)))
        _require(skip.dtype == x.dtype, "mask_head_stage: skip must have x's dtype")
        F, size = skip.shape[0], (skip.shape[2], skip.shape[3])
        _require(F > 0 and size[0] > 0 and size[1] > 0, "mask_head_stage: skip would be empty %s" % (tuple(skip.shape),))
        if skip_index is None:
            _require(F == N, "mask_head_stage: without skip_index skip must have x's %s images, got %s" % (N, F))
        else:
            _require(skip_index.dim() == 1 and skip_index.shape[0] == N, "mask_head_stage: skip_index must be [N] = [%s]" % N)
            _require(skip_index.dtype in (torch.int32, torch.int64), "mask_head_stage: skip_index must be int32 or int64")
    else:
        _require(skip_index is None, "mask_head_stage: skip_index without skip")
    if extra is not None:
        _require(extra.dim() == 4 and extra.shape[0] == N, "mask_head_stage: extra must be [N, E, H, W] = [%s, E, H, W], got %s"
                 % (N, tuple(extra.shape)))
        _mhstage.wide_dtype(x.dtype, extra.dtype, "extra")
        E = extra.shape[1]
        _require(E > 0 and extra.shape[2] > 0 and extra.shape[3] > 0, "mask_head_stage: extra would be empty %s" % (tuple(extra.shape),))
        if size is not None:
            _require(size[0] == extra.shape[2] and size[1] == extra.shape[3],
                     "mask_head_stage: skip %s and extra %s disagree on the output size" % (tuple(skip.shape), tuple(extra.shape)))
        size = (extra.shape[2], extra.shape[3])
    H, W = size if size is not None else (h, w)
    return N, F, C, num_groups, E, h, w, H, W, _mhstage.wide_dtype(x.dtype, out_dtype, "out")


def _dense(t):
    return None if t is None else t.contiguous()


def _forward(x, num_groups, weight, bias, eps, skip=None, skip_index=None, extra=None, out_dtype=None):
    """(out, mean, rstd): out [N, C+E, H, W] in channels-last memory, mean and rstd [N, G] in the arithmetic type."""
    _check_device("mask_head_stage", [("x", x), ("weight", weight), ("bias", bias), ("skip", skip), ("skip_index", skip_index), ("extra", extra)])
    N, F, C, G, E, h, w, H, W, odt = check_shapes(x, num_groups, weight, bias, skip, skip_index, extra, out_dtype)
    acc = _native.acc_dtype(x.dtype)
    out = torch.empty((N, C + E, H, W), dtype=odt, device=x.device, memory_format=torch.channels_last)
    mean, rstd = torch.empty((N, G), dtype=acc, device=x.device), torch.empty((N, G), dtype=acc, device=x.device)
    if N == 0:
        return out, mean, rstd
    shape = _mhstage.Shape(N, F, C, G, E, h, w, H, W)
    code = _native.dtype_code(x.dtype)
    _mhstage.forward(code, weight.dtype != x.dtype, extra is not None and extra.dtype != x.dtype, odt != x.dtype,
                     x.contiguous(), weight.contiguous(), bias.contiguous(), eps, _dense(skip), _dense(skip_index),
                     _dense(extra), shape, _workspace(_mhstage, code, shape, x.device), mean, rstd, out)
    return out, mean, rstd


def _backward(grad_out, x, weight, bias, mean, rstd, skip_index, num_groups, num_skip, grads=NEED_ALL):
    """(grad_x, grad_weight, grad_bias, grad_skip) for the gradients in ``grads``; the others are neither allocated nor
    computed and come back None.  ``num_skip`` is F (0 without a skip).  grad_extra is the slice ``grad_out[:, C:]`` and is
    taken by the caller.  Each gradient alone has the bits it has in a full backward."""
    _require(0 <= grads <= NEED_ALL, "mask_head_stage: grads must be a mask of the NEED_* bits")
    _check_device("mask_head_stage", [("x", x), ("weight", weight), ("bias", bias), ("mean", mean), ("rstd", rstd), ("skip_index", skip_index),
                   ("grad_out", grad_out)])
    _require(x.dim() == 4 and grad_out.dim() == 4 and grad_out.shape[0] == x.shape[0] and grad_out.shape[1] >= x.shape[1],
             "mask_head_stage: grad_out must be [N, C+E, H, W]")
    N, C, h, w = x.shape
    G, E, H, W = num_groups, grad_out.shape[1] - C, grad_out.shape[2], grad_out.shape[3]
    _require(C % G == 0 and tuple(mean.shape) == (N, G) and tuple(rstd.shape) == (N, G), "mask_head_stage: mean and rstd must be [N, G]")
    odt = _mhstage.wide_dtype(x.dtype, grad_out.dtype, "grad_out")
    _mhstage.wide_dtype(x.dtype, weight.dtype, "weight")
    _require(not (grads & NEED_SKIP) or num_skip > 0, "mask_head_stage: grad_skip without a skip")
    grads &= ~NEED_EXTRA
    if grads == 0:
        return None, None, None, None
    dev, acc = x.device, _native.acc_dtype(x.dtype)
    grad_w = torch.empty_like(weight, memory_format=torch.contiguous_format) if grads & NEED_WEIGHT else None
    grad_b = torch.empty_like(bias, memory_format=torch.contiguous_format) if grads & NEED_BIAS else None
    grad_skip = torch.empty((num_skip, C, H, W), dtype=x.dtype, device=dev) if grads & NEED_SKIP else None
    if N == 0:
        for t in (grad_w, grad_b, grad_skip):
            if t is not None:
                t.zero_()
        return (torch.empty_like(x, memory_format=torch.contiguous_format) if grads & NEED_X else None), grad_w, grad_b, grad_skip
    # NCHW (what a convolution hands back) and channels-last (what autograd may pick when it sums formats) are read in
    # place; anything else costs one copy
    channels_last = False
    if not grad_out.is_contiguous():
        channels_last = grad_out.is_contiguous(memory_format=torch.channels_last)
        if not channels_last:
            grad_out = grad_out.contiguous()
    dy = grad_x = None
    if grads & (NEED_X | NEED_WEIGHT | NEED_BIAS):
        dy = torch.empty((N, C, h, w), dtype=acc, device=dev)
        if grads & NEED_X:
            grad_x = dy if acc == x.dtype else torch.empty((N, C, h, w), dtype=x.dtype, device=dev)
    shape = _mhstage.Shape(N, num_skip, C, G, E, h, w, H, W)
    code = _native.dtype_code(x.dtype)
    _mhstage.backward(grads, code, weight.dtype != x.dtype, odt != x.dtype, x.contiguous(), weight.contiguous(),
                      bias.contiguous(), mean, rstd, _dense(skip_index), grad_out, channels_last, shape,
                      _workspace(_mhstage, code, shape, dev), dy, grad_x, grad_w, grad_b, grad_skip)
    return grad_x, grad_w, grad_b, grad_skip


def grad_extra_of(grad_out, num_channels, extra_dtype):
    """grad_extra: the tail channels of grad_out, in extra's dtype."""
    return grad_out[:, num_channels:].to(extra_dtype)


def setup_context(ctx, inputs, output):
    x, num_groups, weight, bias, eps, skip, skip_index, extra = inputs[:8]
    out, mean, rstd = output
    ctx.num_groups = num_groups
    ctx.num_skip = 0 if skip is None else skip.shape[0]
    ctx.extra_dtype = None if extra is None else extra.dtype
    ctx.mark_non_differentiable(mean, rstd)
    ctx.save_for_backward(x, weight, bias, mean, rstd, skip_index)


def backward(run, ctx, grad_out, grad_mean, grad_rstd):
    """The autograd formula; ``run`` is :func:`_backward`, or the backward op with its empty gradients mapped to None."""
    x, weight, bias, mean, rstd, skip_index = ctx.saved_tensors
    need = ctx.needs_input_grad
    grads = grads_mask(need[0], need[2], need[3], need[5], need[7])
    gx, gw, gb, gs = run(grad_out, x, weight, bias, mean, rstd, skip_index, ctx.num_groups, ctx.num_skip, grads)
    ge = grad_extra_of(grad_out, x.shape[1], ctx.extra_dtype) if grads & NEED_EXTRA else None
    return gx, None, gw, gb, None, gs, None, ge, None


class MaskHeadStageFunction(torch.autograd.Function):
    """``mask_head_stage`` for eager code: ``apply(x, num_groups, weight, bias, eps, skip, skip_index, extra, out_dtype)`` ->
    (out, mean, rstd), the last two without a gradient: the formula's ``setup_context`` reads them from the output, as the op's
    does.  Saves x, weight, bias, mean, rstd and skip_index -- not out.  The backward computes the gradients
    ``ctx.needs_input_grad`` names and no others."""
    forward = staticmethod(_forward)
    setup_context = staticmethod(setup_context)
    backward = eager_backward(backward, _backward)
