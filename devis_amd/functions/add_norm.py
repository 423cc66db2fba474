"""Host side of the glue between the transformer layers' GEMMs (include/addnorm.h):
``add_layer_norm(x, delta, weight, bias)`` = ``LayerNorm(x + dropout(delta))`` and ``relu_dropout(x)`` = ``dropout(relu(x))``,
each one kernel pass forward and one backward (two when the parameters' column sums span chunks).  Argument checks, the output
and workspace tensors, the kernel launches and the two autograd Functions.

The dropout mask is a function of ``(seed, row, channel)`` (Philox4x32-10; the rule is in the header): it is never stored, the
backward recomputes it.  ``seed`` is an int64 DEVICE tensor of one element that only the kernels read -- nothing here reads a
device value on the host, and a HIP graph replayed after ``seed.copy_(...)`` draws a new mask.  Every sum has a fixed order and
there are no atomics: every result is bitwise reproducible and nothing here raises or warns under
``torch.use_deterministic_algorithms(True)``.

These two are NOT ``torch.library`` ops.  Inductor fuses exactly this chain on its own, so while
``torch.compiler.is_compiling()`` is true the public functions compute the torch composite --
``F.layer_norm(x + F.dropout(delta, p))`` and ``F.dropout(F.relu(x), p)`` --, whose mask then comes from torch's generator and
IGNORES ``seed``.  Compiled and exported models neither break a graph nor change.

There is no CPU path and no eager fallback: CPU tensors raise, a failing kernel call raises.
"""
import torch
import torch.nn.functional as F

from .. import _addnorm, _native
from ._common import _check_device, _require, eager_backward

DTYPES = (torch.float32, torch.float64, torch.bfloat16, torch.float16)
HALVES = (torch.bfloat16, torch.float16)


def check_p(op, p, seed):
    """The dropout arguments: ``p`` in [0, 1], and a seed -- int64, one element -- when p > 0.  Returns p as a float."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError("%s: dropout probability has to be between 0 and 1, but got %s" % (op, p))
    if p > 0.0:
        if seed is None:
            raise ValueError("%s: p = %s needs a seed (an int64 device tensor of one element)" % (op, p))
        _require(isinstance(seed, torch.Tensor) and seed.dtype == torch.int64 and seed.numel() == 1,
                 "%s: seed must be an int64 tensor of one element" % op)
    return p


def supported(x_dtype, delta_dtype, param_dtype, out_dtype=None):
    """Whether the kernels take this combination of dtypes (include/addnorm.h)."""
    y_dtype = x_dtype if out_dtype is None else out_dtype
    if x_dtype not in DTYPES or delta_dtype not in DTYPES or y_dtype not in DTYPES:
        return False
    if x_dtype == delta_dtype == y_dtype:
        return param_dtype == x_dtype or (x_dtype in HALVES and param_dtype == torch.float32)
    if x_dtype == torch.float32 and delta_dtype in HALVES and y_dtype == torch.float32:
        return param_dtype == torch.float32
    if x_dtype in HALVES and delta_dtype == x_dtype and y_dtype == torch.float32:
        return param_dtype in (x_dtype, torch.float32)
    return False


def check_norm(x, delta, weight, bias, out_dtype):
    """Shape and dtype contract of add_layer_norm; raises before anything is launched.  Works on fake tensors.  Returns
    (R, C, y's dtype).  (The messages are formatted only when they are raised: this runs on every call of a layer.)"""
    op = "add_layer_norm"
    if x.dim() < 1 or x.shape != delta.shape:
        raise RuntimeError("%s: x and delta must have one shape [..., C], got %s and %s" % (op, tuple(x.shape), tuple(delta.shape)))
    C = x.shape[-1]
    if not 1 <= C <= _addnorm.MAX_CHANNELS:
        raise RuntimeError("%s: 1 to %d channels, got %d" % (op, _addnorm.MAX_CHANNELS, C))
    if weight is None or bias is None:
        raise RuntimeError("%s: weight and bias are required" % op)
    if tuple(weight.shape) != (C,) or tuple(bias.shape) != (C,):
        raise RuntimeError("%s: weight and bias must be [%d]" % (op, C))
    if weight.dtype != bias.dtype:
        raise RuntimeError("%s: weight is %s, bias %s" % (op, weight.dtype, bias.dtype))
    if not supported(x.dtype, delta.dtype, weight.dtype, out_dtype):
        raise RuntimeError(
            "%s: unsupported dtypes (x %s, delta %s, parameters %s, out_dtype %s): one dtype of float32 / float64 / bfloat16 / "
            "float16, a 16-bit delta beside float32 x, or 16-bit x and delta with out_dtype=float32; parameters in float32 or "
            "x's dtype" % (op, x.dtype, delta.dtype, weight.dtype, out_dtype))
    return x.numel() // C, C, x.dtype if out_dtype is None else out_dtype


def _forward(x, delta, weight, bias, seed, eps, p, out_dtype, want_stats=True):
    """(y [..., C], mean [...], rstd [...]); the statistics, in the arithmetic type, are None unless ``want_stats``."""
    p = check_p("add_layer_norm", p, seed)
    R, C, y_dtype = check_norm(x, delta, weight, bias, out_dtype)
    seed = seed if p > 0.0 else None
    _check_device("add_layer_norm", [("x", x), ("delta", delta), ("weight", weight), ("bias", bias), ("seed", seed)])
    acc = _native.acc_dtype(x.dtype)
    y = torch.empty(x.shape, dtype=y_dtype, device=x.device)
    mean = torch.empty(x.shape[:-1], dtype=acc, device=x.device) if want_stats else None
    rstd = torch.empty(x.shape[:-1], dtype=acc, device=x.device) if want_stats else None
    if R:
        _addnorm.forward(_addnorm.types_of(x.dtype, delta.dtype, y_dtype, weight.dtype), x.contiguous(), delta.contiguous(),
                         weight.contiguous(), bias.contiguous(), seed, p, eps, _addnorm.Shape(R, C), y, mean, rstd)
    return y, mean, rstd


def _backward(grad_y, x, delta, weight, mean, rstd, seed, p, wants):
    """(grad_x, grad_delta, grad_weight, grad_bias), each in its operand's dtype, None where ``wants`` is False.  One launch (two
    when grad_weight or grad_bias spans chunks); with p == 0 and one dtype grad_delta IS grad_x, with p == 1 it is zeros."""
    op = "add_layer_norm"
    want_x, want_d, want_w, want_b = wants
    _require(any(wants), "%s: no gradient is asked for" % op)
    seed = seed if p > 0.0 else None
    _check_device(op, [("grad_y", grad_y), ("x", x), ("delta", delta), ("weight", weight), ("mean", mean), ("rstd", rstd),
                       ("seed", seed)])
    C = x.shape[-1]
    R = x.numel() // C
    _require(grad_y.shape == x.shape, "%s: the gradient of y must have x's shape" % op)
    shared = want_d and p == 0.0 and delta.dtype == x.dtype         # grad_delta is grad_x
    zero = want_d and p == 1.0
    new = lambda like, on: torch.empty(like.shape, dtype=like.dtype, device=like.device) if on else None      # noqa: E731
    grad_x = new(x, want_x or shared)
    grad_delta = torch.zeros_like(delta) if zero else new(delta, want_d and not shared)
    grad_weight, grad_bias = new(weight, want_w), new(weight, want_b)
    to_x, to_d = grad_x, None if zero else grad_delta
    if R and (to_x is not None or to_d is not None or want_w or want_b):
        shape = _addnorm.Shape(R, C)
        nbytes = _addnorm.workspace_bytes(_native.dtype_code(x.dtype), shape) if want_w or want_b else 0
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
        _addnorm.backward(_addnorm.types_of(x.dtype, delta.dtype, grad_y.dtype, weight.dtype), x.contiguous(), delta.contiguous(),
                          weight.contiguous(), seed, p, mean.contiguous(), rstd.contiguous(), grad_y.contiguous(), shape,
                          workspace, to_x, to_d, grad_weight, grad_bias)
    elif not R:
        for g in (grad_weight, grad_bias):
            if g is not None:
                g.zero_()
    return grad_x if want_x else None, grad_x if shared else grad_delta, grad_weight, grad_bias


def setup_context(ctx, inputs, output):
    x, delta, weight, bias, seed, eps, p, out_dtype = inputs
    y, mean, rstd = output
    ctx.p = float(p)
    ctx.mark_non_differentiable(mean, rstd)
    ctx.save_for_backward(x, delta, weight, mean, rstd, seed if ctx.p > 0.0 else None)


def backward(run, ctx, grad_y, grad_mean, grad_rstd):
    """The autograd formula; ``run`` is :func:`_backward`."""
    wants = tuple(ctx.needs_input_grad[:4])
    if not any(wants):
        return (None,) * 8
    x, delta, weight, mean, rstd, seed = ctx.saved_tensors
    return run(grad_y, x, delta, weight, mean, rstd, seed, ctx.p, wants) + (None,) * 4


class AddLayerNormFunction(torch.autograd.Function):
    """``add_layer_norm`` for eager code: ``apply(x, delta, weight, bias, seed or None, eps, p, out_dtype)`` -> (y, mean, rstd).
    Saves x, delta, weight, mean, rstd and the seed -- not y, not the sum, no mask; only y is differentiable.  The backward
    computes the gradients autograd asks for and launches nothing when it asks for none."""
    @staticmethod
    def forward(x, delta, weight, bias, seed, eps, p, out_dtype):
        return _forward(x, delta, weight, bias, seed, eps, p, out_dtype)

    setup_context = staticmethod(setup_context)
    backward = eager_backward(backward, _backward)


# ---- the relu pass ----------------------------------------------------------------------------------------------------------

def _relu_forward(x, seed, p):
    """y in x's shape and dtype."""
    p = check_p("relu_dropout", p, seed)
    _require(x.dim() >= 1 and x.shape[-1] >= 1, "relu_dropout: x must be [..., C]")
    code = _native.dtype_code(x.dtype)          # raises on an unsupported dtype
    seed = seed if p > 0.0 else None
    _check_device("relu_dropout", [("x", x), ("seed", seed)])
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    if x.numel():
        _addnorm.relu_forward(code, x.contiguous(), seed, p, _addnorm.Shape(x.numel() // x.shape[-1], x.shape[-1]), y)
    return y


def _relu_backward(grad_y, y, p):
    """grad_x = y > 0 ? grad_y * scale : 0, from y alone."""
    _check_device("relu_dropout", [("grad_y", grad_y), ("y", y)])
    _require(grad_y.shape == y.shape and grad_y.dtype == y.dtype, "relu_dropout: the gradient of y must have y's shape and dtype")
    grad_x = torch.empty(y.shape, dtype=y.dtype, device=y.device)
    if y.numel():
        _addnorm.relu_backward(_native.dtype_code(y.dtype), y.contiguous(), grad_y.contiguous(), p, y.numel(), grad_x)
    return grad_x


def relu_setup_context(ctx, inputs, output):
    ctx.p = float(inputs[2])
    ctx.save_for_backward(output)


def relu_backward(run, ctx, grad_y):
    """The autograd formula; ``run`` is :func:`_relu_backward`."""
    if not ctx.needs_input_grad[0]:
        return None, None, None
    y, = ctx.saved_tensors
    return run(grad_y, y, ctx.p), None, None


class ReluDropoutFunction(torch.autograd.Function):
    """``relu_dropout`` for eager code: ``apply(x, seed or None, p)`` -> y.  Saves y alone (the Linear that follows keeps it
    anyway)."""
    forward = staticmethod(_relu_forward)
    setup_context = staticmethod(relu_setup_context)
    backward = eager_backward(relu_backward, _relu_backward)


# ---- the public functions ---------------------------------------------------------------------------------------------------

def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def add_layer_norm(x, delta, weight, bias, eps=1e-5, *, p=0.0, seed=None, out_dtype=None):
    """``LayerNorm(x + dropout_p(delta))`` over the last dimension as one HIP kernel pass (include/addnorm.h): ``x`` and
    ``delta`` ``[..., C]`` with ``1 <= C <= 1024``, ``weight`` and ``bias`` ``[C]``.  One dtype of float32 / float64 / bfloat16 /
    float16 for all, or a 16-bit ``delta`` beside float32 ``x``, or 16-bit ``x`` and ``delta`` with ``out_dtype=torch.float32``;
    the parameters are float32 or ``x``'s dtype.  Arithmetic is float (double for float64), ``y`` is rounded once.

    ``p`` is the probability of dropping (the caller passes 0 in eval mode); ``seed``, an int64 device tensor of one element, is
    required when ``p > 0`` (ValueError otherwise), read by the kernel only, and ignored when ``p == 0``.  The mask is a
    function of (seed, row, channel): the backward recomputes it, and a graph replay after ``seed.copy_`` draws a new one.

    Differentiable in x, delta, weight and bias (once).  While ``torch.compiler.is_compiling()`` this is the torch composite,
    ``F.layer_norm(x + F.dropout(delta, p))``: its mask comes from torch's generator and ``seed`` is ignored."""
    if torch.compiler.is_compiling():
        p = check_p("add_layer_norm", p, seed)
        z = x + (F.dropout(delta, p, True) if p > 0.0 else delta)
        y = F.layer_norm(z, (z.shape[-1],), weight.to(z.dtype), bias.to(z.dtype), eps)
        return y if out_dtype is None else y.to(out_dtype)
    if _wants_grad(x, delta, weight, bias):
        return AddLayerNormFunction.apply(x, delta, weight, bias, seed, eps, p, out_dtype)[0]
    return _forward(x, delta, weight, bias, seed, eps, p, out_dtype, want_stats=False)[0]


def relu_dropout(x, *, p=0.0, seed=None):
    """``dropout_p(relu(x))`` as one HIP kernel pass, in ``x``'s shape and dtype: a dropped element is exactly 0, a kept NaN
    stays NaN.  ``p`` and ``seed`` as in :func:`add_layer_norm` (the mask's row is the flat index over the leading dimensions).
    The backward reads ``y`` alone.  While ``torch.compiler.is_compiling()`` this is ``F.dropout(F.relu(x), p)``, which ignores
    ``seed``."""
    if torch.compiler.is_compiling():
        p = check_p("relu_dropout", p, seed)
        y = F.relu(x)
        return F.dropout(y, p, True) if p > 0.0 else y
    if _wants_grad(x):
        return ReluDropoutFunction.apply(x, seed, p)
    return _relu_forward(x, seed, p)
