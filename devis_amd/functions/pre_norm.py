"""Host side of the glue of the Swin backbone's blocks (include/prenorm.h):
``residual_layer_norm(x, delta, weight, bias)`` = ``s = x + keep * delta``, ``y = LayerNorm(s)``, with ``y`` optionally stored
into the zero-padded window map, and ``patch_merge_norm(x, H, W, weight, bias)`` = the LayerNorm of ``PatchMerging``'s 2 x 2
gather -- each one kernel pass forward and one backward (two when the parameters' column sums span chunks).  Argument checks,
the output and workspace tensors, the kernel launches and the two autograd Functions.

Every sum has a fixed order and there are no atomics: every result is bitwise reproducible and nothing here raises or warns
under ``torch.use_deterministic_algorithms(True)``.

These two are NOT ``torch.library`` ops, for the reason DESIGN.md section 19 gives for ``add_layer_norm``: Inductor fuses exactly
this chain on its own.  The public functions compute the TORCH COMPOSITE -- the reference's chain of ``F.layer_norm``,
``F.pad``, slices and ``cat`` -- while ``torch.compiler.is_compiling()``, on CPU tensors, in float64 or another dtype mix the
kernels do not take, and above ``PRENORM_MAX_CHANNELS`` channels.  On the kernel route a failing call raises.
"""
import torch
import torch.nn.functional as F

from .. import _prenorm
from ._common import _check_device, _require

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
HALVES = (torch.bfloat16, torch.float16)


def _on_gpu(t):
    return t.is_cuda


def supported(x_dtype, delta_dtype, param_dtype, y_dtype):
    """Whether the kernels take this combination of dtypes (include/prenorm.h); ``delta_dtype`` is x's without a delta."""
    if x_dtype not in DTYPES or delta_dtype not in DTYPES or y_dtype not in DTYPES or param_dtype not in DTYPES:
        return False
    if x_dtype == torch.float32:
        halves = {d for d in (delta_dtype, y_dtype) if d in HALVES}
        return param_dtype == torch.float32 and len(halves) <= 1
    return delta_dtype == x_dtype and y_dtype == x_dtype and param_dtype in (x_dtype, torch.float32)


def _geometry(op, x, map_size):
    """(B, H, W, Hp, Wp) of ``x [B, ..., C]``: the tokens of an entry as one row of them unless a map is asked for."""
    _require(x.dim() >= 1 and x.shape[-1] >= 1, "%s: x must be [..., C]" % op)
    C = x.shape[-1]
    B = x.shape[0] if x.dim() >= 2 else 1
    L = x.numel() // (B * C) if B else 0
    if map_size is None:
        return B, 1, L, 0, 0
    H, W, Hp, Wp = (int(v) for v in map_size)
    _require(x.dim() == 3 and L == H * W, "%s: map_size needs x [B, H * W, C], got %s for H, W = %d, %d" % (op, tuple(x.shape), H, W))
    _require(Hp >= H and Wp >= W, "%s: the map (%d x %d) is smaller than H x W = %d x %d" % (op, Hp, Wp, H, W))
    return B, H, W, Hp, Wp


def _check_params(op, C, weight, bias):
    _require(weight is not None and bias is not None, "%s: weight and bias are required" % op)
    _require(tuple(weight.shape) == (C,) and tuple(bias.shape) == (C,), "%s: weight and bias must be [%d]" % (op, C))
    _require(weight.dtype == bias.dtype, "%s: weight is %s, bias %s" % (op, weight.dtype, bias.dtype))


def _check_keep(op, keep, B):
    _require(keep.numel() == B, "%s: keep must have one value per batch entry (%d), got %s" % (op, B, tuple(keep.shape)))
    return keep.reshape(B).to(torch.float32).contiguous()


def _workspace(shape, device, wanted):
    nbytes = _prenorm.workspace_bytes(shape) if wanted else 0
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


# ---- residual_layer_norm ----------------------------------------------------------------------------------------------------

def _forward(x, delta, weight, bias, keep, eps, map_size, out_dtype, want_stats=True):
    """(s or None, y, mean, rstd) of the PLAIN (``delta`` None) or RESIDUAL form; the float32 statistics are None unless
    ``want_stats``."""
    op = "residual_layer_norm"
    B, H, W, Hp, Wp = _geometry(op, x, map_size)
    C = x.shape[-1]
    residual = delta is not None
    y_dtype = x.dtype if out_dtype is None else out_dtype
    _check_device(op, [("x", x), ("delta", delta), ("weight", weight), ("bias", bias), ("keep", keep)])
    shape = _prenorm.Shape(B, H, W, C, Hp, Wp, _prenorm.RESIDUAL if residual else _prenorm.PLAIN,
                           _prenorm.TOKENS if map_size is None else _prenorm.MAP)
    y = torch.empty(x.shape if map_size is None else (B, Hp, Wp, C), dtype=y_dtype, device=x.device)
    s = torch.empty(x.shape, dtype=x.dtype, device=x.device) if residual else None
    mean = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device) if want_stats else None
    rstd = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device) if want_stats else None
    types = _prenorm.types_of(x.dtype, delta.dtype if residual else x.dtype, y_dtype, weight.dtype)
    _prenorm.forward(types, x.contiguous(), delta.contiguous() if residual else None, keep, weight.contiguous(),
                     bias.contiguous(), eps, shape, s, y, mean, rstd)
    return s, y, mean, rstd


def _backward(grad_y, grad_s, z, weight, mean, rstd, keep, geometry, residual, delta_dtype, wants):
    """(grad_x, grad_delta, grad_weight, grad_bias), each in its operand's dtype, None where ``wants`` is False.  ``z`` is the
    forward's ``s`` (``x`` in the PLAIN form).  One launch (two when grad_weight or grad_bias spans chunks); without ``keep``
    and with one dtype grad_delta IS grad_x.  Without ``grad_y`` -- ``y`` was not used -- nothing is launched."""
    op = "residual_layer_norm"
    want_x, want_d, want_w, want_b = wants
    B, H, W, Hp, Wp = geometry
    if grad_y is None:
        grad_delta = None
        if want_d:
            grad_delta = grad_s if keep is None else grad_s * keep.to(grad_s.dtype).view((B,) + (1,) * (grad_s.dim() - 1))
            grad_delta = grad_delta.to(delta_dtype)
        return grad_s if want_x else None, grad_delta, None, None
    _check_device(op, [("grad_y", grad_y), ("grad_s", grad_s), ("s", z), ("weight", weight), ("mean", mean), ("rstd", rstd),
                       ("keep", keep)])
    C = z.shape[-1]
    is_map = Hp > 0
    _require(tuple(grad_y.shape) == ((B, Hp, Wp, C) if is_map else tuple(z.shape)), "%s: the gradient of y must have y's shape" % op)
    _require(grad_s is None or (grad_s.shape == z.shape and grad_s.dtype == z.dtype), "%s: the gradient of s must be like s" % op)
    shared = want_d and keep is None and delta_dtype == z.dtype         # grad_delta is grad_x
    new = lambda shape, dtype, on: torch.empty(shape, dtype=dtype, device=z.device) if on else None      # noqa: E731
    grad_x = new(z.shape, z.dtype, want_x or shared)
    grad_delta = new(z.shape, delta_dtype, want_d and not shared)
    grad_weight, grad_bias = new(weight.shape, weight.dtype, want_w), new(weight.shape, weight.dtype, want_b)
    shape = _prenorm.Shape(B, H, W, C, Hp, Wp, _prenorm.RESIDUAL if residual else _prenorm.PLAIN,
                           _prenorm.MAP if is_map else _prenorm.TOKENS)
    workspace = _workspace(shape, z.device, want_w or want_b)
    _prenorm.backward(_prenorm.types_of(z.dtype, delta_dtype, grad_y.dtype, weight.dtype), z.contiguous(), keep,
                      weight.contiguous(), mean.contiguous(), rstd.contiguous(), grad_y.contiguous(),
                      None if grad_s is None else grad_s.contiguous(), shape, workspace, grad_x, grad_delta, grad_weight, grad_bias)
    return grad_x if want_x else None, grad_x if shared else grad_delta, grad_weight, grad_bias


class ResidualLayerNormFunction(torch.autograd.Function):
    """``residual_layer_norm`` for eager code: ``apply(x, delta or None, weight, bias, keep or None, eps, map_size, out_dtype)``
    -> (s or None, y, mean, rstd).  Saves s (x without a delta), weight, mean, rstd and keep -- never y; s and y are
    differentiable, and the gradient of an output that was not used is not materialised.  The backward computes the gradients
    autograd asks for and launches nothing when it asks for none."""
    @staticmethod
    def forward(x, delta, weight, bias, keep, eps, map_size, out_dtype):
        return _forward(x, delta, weight, bias, keep, eps, map_size, out_dtype)

    @staticmethod
    def setup_context(ctx, inputs, output):
        x, delta, weight, bias, keep, eps, map_size, out_dtype = inputs
        s, y, mean, rstd = output
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(mean, rstd)
        ctx.residual = delta is not None
        ctx.delta_dtype = delta.dtype if ctx.residual else x.dtype
        ctx.geometry = _geometry("residual_layer_norm", x, map_size)
        ctx.save_for_backward(s if ctx.residual else x, weight, mean, rstd, keep)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_s, grad_y, grad_mean, grad_rstd):
        wants = tuple(ctx.needs_input_grad[:4])
        if not any(wants) or (grad_s is None and grad_y is None):
            return (None,) * 8
        z, weight, mean, rstd, keep = ctx.saved_tensors
        return _backward(grad_y, grad_s, z, weight, mean, rstd, keep, ctx.geometry, ctx.residual, ctx.delta_dtype, wants) + (None,) * 4


# ---- patch_merge_norm -------------------------------------------------------------------------------------------------------

def _merge_shape(B, H, W, C):
    return _prenorm.Shape(B, H, W, 4 * C, 0, 0, _prenorm.MERGE, _prenorm.TOKENS)


def _merge_forward(x, weight, bias, H, W, eps, out_dtype, want_stats=True):
    """(y [B, H2 * W2, 4 C], mean, rstd) from x [B, H * W, C]."""
    op = "patch_merge_norm"
    B, L, C = x.shape
    _check_device(op, [("x", x), ("weight", weight), ("bias", bias)])
    rows = ((H + 1) // 2) * ((W + 1) // 2)
    y_dtype = x.dtype if out_dtype is None else out_dtype
    y = torch.empty((B, rows, 4 * C), dtype=y_dtype, device=x.device)
    mean = torch.empty((B, rows), dtype=torch.float32, device=x.device) if want_stats else None
    rstd = torch.empty((B, rows), dtype=torch.float32, device=x.device) if want_stats else None
    _prenorm.forward(_prenorm.types_of(x.dtype, x.dtype, y_dtype, weight.dtype), x.contiguous(), None, None, weight.contiguous(),
                     bias.contiguous(), eps, _merge_shape(B, H, W, C), None, y, mean, rstd)
    return y, mean, rstd


def _merge_backward(grad_y, x, weight, mean, rstd, H, W, wants):
    """(grad_x [B, H * W, C] -- a permutation of the rows' gradients, every element written --, grad_weight, grad_bias)."""
    op = "patch_merge_norm"
    want_x, want_w, want_b = wants
    _check_device(op, [("grad_y", grad_y), ("x", x), ("weight", weight), ("mean", mean), ("rstd", rstd)])
    B, L, C = x.shape
    _require(tuple(grad_y.shape) == (B, mean.shape[1], 4 * C), "%s: the gradient of y must have y's shape" % op)
    new = lambda like, on: torch.empty(like.shape, dtype=like.dtype, device=like.device) if on else None      # noqa: E731
    grad_x, grad_weight, grad_bias = new(x, want_x), new(weight, want_w), new(weight, want_b)
    shape = _merge_shape(B, H, W, C)
    workspace = _workspace(shape, x.device, want_w or want_b)
    _prenorm.backward(_prenorm.types_of(x.dtype, x.dtype, grad_y.dtype, weight.dtype), x.contiguous(), None, weight.contiguous(),
                      mean.contiguous(), rstd.contiguous(), grad_y.contiguous(), None, shape, workspace, grad_x, None, grad_weight,
                      grad_bias)
    return grad_x, grad_weight, grad_bias


class PatchMergeNormFunction(torch.autograd.Function):
    """``patch_merge_norm`` for eager code: ``apply(x, weight, bias, H, W, eps, out_dtype)`` -> (y, mean, rstd).  Saves x, weight,
    mean and rstd -- not y, no gathered tensor: the backward gathers x again."""
    @staticmethod
    def forward(x, weight, bias, H, W, eps, out_dtype):
        return _merge_forward(x, weight, bias, H, W, eps, out_dtype)

    @staticmethod
    def setup_context(ctx, inputs, output):
        x, weight, bias, H, W, eps, out_dtype = inputs
        y, mean, rstd = output
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(mean, rstd)
        ctx.size = (H, W)
        ctx.save_for_backward(x, weight, mean, rstd)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y, grad_mean, grad_rstd):
        wants = tuple(ctx.needs_input_grad[:3])
        if not any(wants) or grad_y is None:
            return (None,) * 7
        x, weight, mean, rstd = ctx.saved_tensors
        return _merge_backward(grad_y, x, weight, mean, rstd, ctx.size[0], ctx.size[1], wants) + (None,) * 4


# ---- the torch composites ---------------------------------------------------------------------------------------------------

def _norm(z, weight, bias, eps, out_dtype):
    y = F.layer_norm(z, (z.shape[-1],), weight, bias, eps)
    return y if out_dtype is None else y.to(out_dtype)


def residual_layer_norm_composite(x, delta, weight, bias, eps=1e-5, *, keep=None, map_size=None, out_dtype=None):
    """What :func:`residual_layer_norm` computes, by torch: the reference's ``x + drop_path(delta)``, ``norm(...)`` and
    ``F.pad``."""
    s = x
    if delta is not None:
        s = x + (delta if keep is None else delta * keep.to(delta.dtype).view((x.shape[0],) + (1,) * (x.dim() - 1)))
    y = _norm(s, weight, bias, eps, out_dtype)
    if map_size is not None:
        B, H, W, Hp, Wp = _geometry("residual_layer_norm", x, map_size)
        y = F.pad(y.view(B, H, W, x.shape[-1]), (0, 0, 0, Wp - W, 0, Hp - H))
    return s, y


def patch_merge_norm_composite(x, H, W, weight, bias, eps=1e-5, *, out_dtype=None):
    """What :func:`patch_merge_norm` computes, by torch: ``PatchMerging.forward`` up to its Linear."""
    B, L, C = x.shape
    x = x.view(B, H, W, C)
    if H % 2 == 1 or W % 2 == 1:
        x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    x = torch.cat([x[:, 0::2, 0::2, :], x[:, 1::2, 0::2, :], x[:, 0::2, 1::2, :], x[:, 1::2, 1::2, :]], -1)
    return _norm(x.view(B, -1, 4 * C), weight, bias, eps, out_dtype)


# ---- the public functions ---------------------------------------------------------------------------------------------------

def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def takes_kernels(x, delta, weight, C, out_dtype):
    """Whether a call goes to the kernels: not while compiling, not on the CPU, not without elements, at most
    ``PRENORM_MAX_CHANNELS`` channels per row and a dtype mix of include/prenorm.h."""
    if torch.compiler.is_compiling() or not _on_gpu(x) or x.numel() == 0 or not 1 <= C <= _prenorm.MAX_CHANNELS:
        return False
    return supported(x.dtype, x.dtype if delta is None else delta.dtype, weight.dtype, x.dtype if out_dtype is None else out_dtype)


def residual_layer_norm(x, delta, weight, bias, eps=1e-5, *, keep=None, map_size=None, out_dtype=None):
    """``s = x + keep * delta``, ``y = LayerNorm(s)`` over the last dimension as one HIP kernel pass (include/prenorm.h); returns
    ``(s, y)``.  ``x`` and ``delta`` ``[B, ..., C]`` with ``1 <= C <= 3072``, ``weight`` and ``bias`` ``[C]``.  With
    ``delta=None`` nothing is added and ``s is x``.

    ``keep`` ``[B]`` is the drop-path scale of each batch entry -- 0 or ``1 / keep_prob`` --, data and not a differentiable
    operand; None means 1.  An entry with ``keep == 0`` takes exactly ``x``, whatever ``delta`` holds there.
    ``map_size=(H, W, Hp, Wp)``, for ``x [B, H * W, C]``, makes ``y`` the map ``[B, Hp, Wp, C]`` with the tokens at
    ``[:, :H, :W]`` and exactly 0 elsewhere (``norm1`` and ``F.pad`` in one pass).  ``out_dtype`` is ``y``'s dtype: a 16-bit one
    beside float32 ``x`` is what an autocast Linear reads without a cast pass.

    dtypes: one of float32 / bfloat16 / float16 for all; beside float32 ``x`` and parameters a 16-bit ``delta``, a 16-bit ``y``
    or both; float32 parameters beside 16-bit tensors.  Arithmetic is float32, ``s`` and ``y`` are rounded once.  Differentiable
    in x, delta, weight and bias (once), through ``s`` and ``y``.  On the CPU, in float64 or another dtype mix, above 3072
    channels and while ``torch.compiler.is_compiling()`` this is the torch composite."""
    C = x.shape[-1]
    _check_params("residual_layer_norm", C, weight, bias)
    _require(delta is None or delta.shape == x.shape, "residual_layer_norm: x and delta must have one shape [..., C]")
    _require(keep is None or delta is not None, "residual_layer_norm: keep scales delta, and there is none")
    if not takes_kernels(x, delta, weight, C, out_dtype):
        return residual_layer_norm_composite(x, delta, weight, bias, eps, keep=keep, map_size=map_size, out_dtype=out_dtype)
    if keep is not None:
        keep = _check_keep("residual_layer_norm", keep.detach(), x.shape[0] if x.dim() >= 2 else 1)
    if _wants_grad(x, delta, weight, bias):
        s, y = ResidualLayerNormFunction.apply(x, delta, weight, bias, keep, eps, map_size, out_dtype)[:2]
    else:
        s, y = _forward(x, delta, weight, bias, keep, eps, map_size, out_dtype, want_stats=False)[:2]
    return (x if delta is None else s), y


def patch_merge_norm(x, H, W, weight, bias, eps=1e-5, *, out_dtype=None):
    """The LayerNorm of ``PatchMerging``'s 2 x 2 gather as one HIP kernel pass (include/prenorm.h): ``x [B, H * W, C]`` ->
    ``y [B, ceil(H / 2) * ceil(W / 2), 4 C]``, whose row ``(i, j)`` is the norm of the concatenation of ``x[2i, 2j]``,
    ``x[2i+1, 2j]``, ``x[2i, 2j+1]`` and ``x[2i+1, 2j+1]`` (0 outside ``H x W``); ``weight`` and ``bias`` ``[4 C]`` with
    ``4 C <= 3072``.  No padded, sliced or concatenated tensor exists, forward or backward.  dtypes and the composite route as in
    :func:`residual_layer_norm`."""
    _require(x.dim() == 3 and x.shape[1] == H * W, "patch_merge_norm: x must be [B, H * W, C], got %s for H, W = %d, %d" % (tuple(x.shape), H, W))
    C = x.shape[-1]
    _check_params("patch_merge_norm", 4 * C, weight, bias)
    if not takes_kernels(x, None, weight, 4 * C, out_dtype):
        return patch_merge_norm_composite(x, H, W, weight, bias, eps, out_dtype=out_dtype)
    if _wants_grad(x, weight, bias):
        return PatchMergeNormFunction.apply(x, weight, bias, H, W, eps, out_dtype)[0]
    return _merge_forward(x, weight, bias, H, W, eps, out_dtype, want_stats=False)[0]
