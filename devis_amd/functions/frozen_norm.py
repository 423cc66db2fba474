"""Host side of the glue of the ResNet backbone's blocks (include/frozennorm.h):
``frozen_batch_norm(x, weight, bias, running_mean, running_var)`` = the reference's ``FrozenBatchNorm2d`` with, optionally, the
shortcut add (whose own frozen norm folds in) and the ReLU behind it, and ``frozen_batch_norm_relu_pool`` = the stem's norm,
ReLU and 3 x 3 / stride 2 max-pool -- each one kernel pass forward; the first has a one-pass backward.  Argument checks, the
output tensors, the kernel launches and the autograd Function.

Nothing is reduced and there are no atomics: every result is bitwise reproducible and nothing here raises or warns under
``torch.use_deterministic_algorithms(True)``.

These are NOT ``torch.library`` ops, for the reason DESIGN.md section 19 gives for ``add_layer_norm``: Inductor fuses exactly
this chain on its own.  The public functions compute the TORCH COMPOSITE -- the reference's ``x * scale + bias`` and the stock
``relu`` / ``max_pool2d`` -- while ``torch.compiler.is_compiling()``, on CPU tensors, in float64 or another dtype the kernels do
not take, with buffers that are not float32, in a layout that is neither contiguous NCHW nor contiguous channels-last, with
``x`` and ``residual`` in different layouts, and -- the pool -- when ``x`` requires grad.  On the kernel route a failing call
raises.
"""
import torch
import torch.nn.functional as F

from .. import _frozennorm
from ._common import _check_device, _require

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
HALVES = (torch.bfloat16, torch.float16)
BUFFER_DTYPES = (torch.float32,)
NCHW, NHWC = _frozennorm.NCHW, _frozennorm.NHWC


def _on_gpu(t):
    return t.is_cuda


def layouts_of(t):
    """The layouts a 4-D tensor's memory is: a set of NCHW / NHWC (both for a tensor with C == 1 or H * W == 1)."""
    found = set()
    if t.dim() == 4:
        if t.is_contiguous():
            found.add(NCHW)
        if t.is_contiguous(memory_format=torch.channels_last):
            found.add(NHWC)
    return found


def common_layout(*tensors):
    """The one layout all of ``tensors`` (None entries skipped) are in -- NCHW where both fit --, or None."""
    found = {NCHW, NHWC}
    for t in tensors:
        if t is not None:
            found &= layouts_of(t)
    return NCHW if NCHW in found else (NHWC if found else None)


def _norm_of(op, C, weight, bias, running_mean, running_var, eps):
    for name, t in (("weight", weight), ("bias", bias), ("running_mean", running_mean), ("running_var", running_var)):
        _require(isinstance(t, torch.Tensor) and tuple(t.shape) == (C,), "%s: %s must be a tensor [%d]" % (op, name, C))
    _require(weight.dtype == bias.dtype == running_mean.dtype == running_var.dtype, "%s: the four buffers must have one dtype" % op)
    return (weight, bias, running_mean, running_var, float(eps))


def _detached(norm):
    return None if norm is None else tuple(t.detach().contiguous() for t in norm[:4]) + (norm[4],)


def _empty(shape, dtype, device, layout):
    return torch.empty(tuple(shape), dtype=dtype, device=device,
                       memory_format=torch.channels_last if layout == NHWC else torch.contiguous_format)


def _in_layout(t, layout):
    return t.contiguous(memory_format=torch.channels_last if layout == NHWC else torch.contiguous_format)


def _shape(x, layout, form, relu):
    N, C, H, W = x.shape
    return _frozennorm.Shape(N, C, H, W, layout, form, int(bool(relu)))


def _form(residual, residual_norm):
    return _frozennorm.NONE if residual is None else (_frozennorm.PLAIN if residual_norm is None else _frozennorm.NORMED)


# ---- frozen_batch_norm ------------------------------------------------------------------------------------------------------

def _forward(x, norm, residual, residual_norm, relu, y_dtype, layout):
    op = "frozen_batch_norm"
    _check_device(op, [("x", x), ("residual", residual)] + [("a buffer", t) for n in (norm, residual_norm) if n for t in n[:4]])
    y = _empty(x.shape, y_dtype, x.device, layout)
    types = _frozennorm.types_of(x.dtype, x.dtype if residual is None else residual.dtype, y_dtype)
    _frozennorm.forward(types, _shape(x, layout, _form(residual, residual_norm), relu), x, norm, residual, residual_norm, y)
    return y


def _backward(grad_y, y, norm, residual_norm, form, relu, x_dtype, r_dtype, layout, wants):
    """(grad_x, grad_residual), each in its operand's dtype, None where ``wants`` is False: one launch."""
    op = "frozen_batch_norm"
    want_x, want_r = wants
    _check_device(op, [("grad_y", grad_y), ("y", y)])
    grad_y = _in_layout(grad_y, layout)
    grad_x = _empty(grad_y.shape, x_dtype, grad_y.device, layout) if want_x else None
    grad_r = _empty(grad_y.shape, r_dtype, grad_y.device, layout) if want_r else None
    types = _frozennorm.types_of(x_dtype, r_dtype, grad_y.dtype)
    _frozennorm.backward(types, _shape(grad_y, layout, form, relu), grad_y, y if relu else None, norm if want_x else None,
                         residual_norm if want_r and form == _frozennorm.NORMED else None, grad_x, grad_r)
    return grad_x, grad_r


class FrozenNormFunction(torch.autograd.Function):
    """``frozen_batch_norm`` for eager code: ``apply(x, norm, residual or None, residual_norm or None, relu, y_dtype, layout)``
    -> y, with ``norm`` = (weight, bias, running_mean, running_var, eps) of detached buffers.  Saves ``y`` when there is a ReLU
    and nothing otherwise; the backward computes the gradients autograd asks for, in one launch."""
    @staticmethod
    def forward(x, norm, residual, residual_norm, relu, y_dtype, layout):
        return _forward(x, norm, residual, residual_norm, relu, y_dtype, layout)

    @staticmethod
    def setup_context(ctx, inputs, output):
        x, norm, residual, residual_norm, relu, y_dtype, layout = inputs
        ctx.set_materialize_grads(False)
        ctx.norm, ctx.residual_norm, ctx.relu, ctx.layout = norm, residual_norm, bool(relu), layout
        ctx.form = _form(residual, residual_norm)
        ctx.x_dtype, ctx.r_dtype = x.dtype, x.dtype if residual is None else residual.dtype
        if relu:
            ctx.save_for_backward(output)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        wants = (ctx.needs_input_grad[0], ctx.needs_input_grad[2])
        if not any(wants) or grad_y is None:
            return (None,) * 7
        y = ctx.saved_tensors[0] if ctx.relu else None
        grad_x, grad_r = _backward(grad_y, y, ctx.norm, ctx.residual_norm, ctx.form, ctx.relu, ctx.x_dtype, ctx.r_dtype,
                                   ctx.layout, wants)
        return grad_x, None, grad_r, None, None, None, None


# ---- frozen_batch_norm_relu_pool --------------------------------------------------------------------------------------------

def pooled(n):
    """The extent ``max_pool2d(kernel 3, stride 2, padding 1)`` makes of ``n``."""
    return (n - 1) // 2 + 1 if n > 0 else 0


def _pool_forward(x, norm, y_dtype, layout):
    op = "frozen_batch_norm_relu_pool"
    _check_device(op, [("x", x)] + [("a buffer", t) for t in norm[:4]])
    N, C, H, W = x.shape
    y = _empty((N, C, pooled(H), pooled(W)), y_dtype, x.device, layout)
    _frozennorm.pool_forward(_frozennorm.types_of(x.dtype, x.dtype, y_dtype), _shape(x, layout, _frozennorm.NONE, True), x, norm, y)
    return y


# ---- the torch composites ---------------------------------------------------------------------------------------------------

def _affine(x, weight, bias, running_mean, running_var, eps):
    """The frozen norm as torch computes it: the per-channel constants ``s`` and ``t`` of include/frozennorm.h as [C] vectors,
    then a product and a sum over the map (the stock module's operation order, not the kernels' fma)."""
    s = torch.rsqrt(running_var + eps) * weight
    t = bias - s * running_mean
    per_channel = (1, x.shape[1], 1, 1)
    return x * s.view(per_channel) + t.view(per_channel)


def frozen_batch_norm_composite(x, weight, bias, running_mean, running_var, eps=1e-5, residual=None, residual_norm=None,
                                relu=False, out_dtype=None):
    """What :func:`frozen_batch_norm` computes, by torch."""
    y = _affine(x, weight, bias, running_mean, running_var, eps)
    if residual is not None:
        y = y + (residual if residual_norm is None else _affine(residual, *residual_norm))
    if relu:
        y = torch.relu(y)
    return y if out_dtype is None else y.to(out_dtype)


def frozen_batch_norm_relu_pool_composite(x, weight, bias, running_mean, running_var, eps=1e-5, out_dtype=None):
    """What :func:`frozen_batch_norm_relu_pool` computes, by torch."""
    y = F.max_pool2d(torch.relu(_affine(x, weight, bias, running_mean, running_var, eps)), kernel_size=3, stride=2, padding=1)
    return y if out_dtype is None else y.to(out_dtype)


# ---- the public functions ---------------------------------------------------------------------------------------------------

def eligible(x, *norms):
    """Whether a call on ``x`` with these norms -- ``(weight, bias, running_mean, running_var, ...)`` each -- can go to the
    kernels at all: not while compiling, a 4-D GPU tensor with elements in a kernel dtype, float32 buffers."""
    if torch.compiler.is_compiling() or not isinstance(x, torch.Tensor) or x.dim() != 4 or x.numel() == 0:
        return False
    if not _on_gpu(x) or x.dtype not in DTYPES:
        return False
    return all(t.dtype in BUFFER_DTYPES for norm in norms for t in norm[:4])


def _takes_kernels(x, norm, residual, residual_norm, y_dtype):
    if not eligible(x, *(n for n in (norm, residual_norm) if n is not None)) or y_dtype not in DTYPES:
        return None
    if residual is not None and (residual.dtype not in DTYPES or not _on_gpu(residual)):
        return None
    if len({d for d in (x.dtype, y_dtype, None if residual is None else residual.dtype) if d in HALVES}) > 1:
        return None
    return common_layout(x, residual)


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def frozen_batch_norm(x, weight, bias, running_mean, running_var, eps=1e-5, residual=None, residual_norm=None, relu=False,
                      out_dtype=None):
    """``y = act(x * s + t + R)`` per channel of ``x [N, C, H, W]`` as one HIP kernel pass (include/frozennorm.h), with
    ``s = weight * rsqrt(running_var + eps)`` and ``t = bias - running_mean * s`` built inside the kernel from the four frozen
    buffers ``[C]``.  ``R`` is nothing, ``residual`` (``x``'s shape), or -- with ``residual_norm = (weight, bias, running_mean,
    running_var, eps)``, the frozen norm of a block's ``downsample`` branch -- ``residual * s2 + t2``.  ``relu=True`` applies
    ``torch.relu`` (NaN propagates).

    ``x`` and ``residual`` are contiguous NCHW or contiguous channels-last, both the same; ``y`` has that layout.  dtypes:
    float32 / bfloat16 / float16, for ``x``, ``residual`` and ``y`` each on its own (bfloat16 and float16 do not mix); the
    buffers are float32; arithmetic is float32 and ``y`` is rounded once.  ``out_dtype=None`` is torch's promotion of ``x``, the
    buffers and ``residual`` -- what the stock modules return: float32 on the kernel route.  Differentiable (once) in ``x`` and
    ``residual``; the buffers are frozen.  Only ``y`` is kept for the backward, and only behind a ReLU.  The module docstring
    lists when this is the torch composite."""
    op = "frozen_batch_norm"
    _require(isinstance(x, torch.Tensor) and x.dim() == 4, "%s: x must be [N, C, H, W]" % op)
    C = x.shape[1]
    norm = _norm_of(op, C, weight, bias, running_mean, running_var, eps)
    _require(residual_norm is None or residual is not None, "%s: residual_norm normalises residual, and there is none" % op)
    _require(residual is None or residual.shape == x.shape, "%s: x and residual must have one shape" % op)
    if residual_norm is not None:
        _require(len(residual_norm) in (4, 5), "%s: residual_norm is (weight, bias, running_mean, running_var, eps)" % op)
        residual_norm = _norm_of(op, C, *residual_norm[:4], residual_norm[4] if len(residual_norm) == 5 else 1e-5)
    y_dtype = out_dtype
    if y_dtype is None:
        y_dtype = torch.promote_types(x.dtype, weight.dtype)
        if residual is not None:
            y_dtype = torch.promote_types(y_dtype, residual.dtype)
            if residual_norm is not None:
                y_dtype = torch.promote_types(y_dtype, residual_norm[0].dtype)
    layout = _takes_kernels(x, norm, residual, residual_norm, y_dtype)
    if layout is None:
        return frozen_batch_norm_composite(x, *norm, residual=residual, residual_norm=residual_norm, relu=relu, out_dtype=out_dtype)
    norm, residual_norm = _detached(norm), _detached(residual_norm)
    if _wants_grad(x, residual):
        return FrozenNormFunction.apply(x, norm, residual, residual_norm, bool(relu), y_dtype, layout)
    return _forward(x.detach(), norm, None if residual is None else residual.detach(), residual_norm, relu, y_dtype, layout)


def frozen_batch_norm_relu_pool(x, weight, bias, running_mean, running_var, eps=1e-5, out_dtype=None):
    """``max_pool2d(relu(x * s + t), kernel_size=3, stride=2, padding=1)`` of the ResNet stem as one HIP kernel pass
    (include/frozennorm.h): ``x [N, C, H, W]`` -> ``[N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1]``; the full-resolution
    normalised map never exists.  Every tap goes through the affine map before the maximum (a negative ``s`` reverses the
    order); NaN propagates as in ``F.max_pool2d``.  Layouts, dtypes and ``out_dtype`` as in :func:`frozen_batch_norm`.  Forward
    only: when ``x`` requires grad this is the torch composite (the reference freezes the stem), as in the other cases the
    module docstring lists."""
    op = "frozen_batch_norm_relu_pool"
    _require(isinstance(x, torch.Tensor) and x.dim() == 4, "%s: x must be [N, C, H, W]" % op)
    norm = _norm_of(op, x.shape[1], weight, bias, running_mean, running_var, eps)
    y_dtype = torch.promote_types(x.dtype, weight.dtype) if out_dtype is None else out_dtype
    layout = None if _wants_grad(x) else _takes_kernels(x, norm, None, None, y_dtype)
    if layout is None:
        return frozen_batch_norm_relu_pool_composite(x, *norm, out_dtype=out_dtype)
    return _pool_forward(x.detach(), _detached(norm), y_dtype, layout)
