"""Host side of the Swin backbone's (shifted-)window attention (include/winattn.h):
``window_attention(qkv, bias_table, num_heads, window_size, shift_size)`` is what a ``SwinTransformerBlock`` computes between
its ``qkv`` Linear and its ``proj`` Linear -- cyclic shift, window partition, scaled logits, relative-position bias, shift mask,
softmax, product with ``v``, window merge and reverse shift -- on the padded map in map order, one kernel pass forward and two
to five backward.  Argument checks, the output tensors, the kernel launches and the autograd Function.

``qkv [B, Hp, Wp, 3C]`` is read where it lies and ``out [B, Hp, Wp, C]`` is written where it belongs: pad, roll, partition,
reverse, roll and slice are index arithmetic in the kernels.  No window copy, no ``[windows, heads, N, N]`` tensor, no mask
tensor and no index buffer exists: the Function saves ``qkv``, the table, ``out`` in float32 (for 16-bit operands a copy the
forward writes before it rounds) and one float32 per row (``lse``), and the backward recomputes the rest.  The table's gradient
is summed without atomics, in an order the shape alone fixes: every result is bitwise reproducible and nothing here raises or
warns under ``torch.use_deterministic_algorithms(True)``.

This is NOT a ``torch.library`` op.  While ``torch.compiler.is_compiling()`` is true the public function computes the torch
composite -- roll, partition, ``matmul``, ``softmax``, ``matmul``, reverse, roll.  Compiled and exported models neither break a
graph nor change.

There is no CPU path and no eager fallback: CPU tensors raise, a failing kernel call raises.
"""
import torch

from .. import _native, _winattn
from ._common import _check_device, _require, eager_backward

OP = "window_attention"
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
MASKED = -100.0                         # the shift mask: finite and additive, as in the reference
_MAX31 = (1 << 31) - 1


def supported(dtype, head_dim, window_size):
    """Whether the kernels take this storage dtype, this many channels per head and this window (include/winattn.h)."""
    return (dtype in DTYPES and head_dim % 4 == 0 and 4 <= head_dim <= _winattn.MAX_HEAD_DIM and
            1 <= window_size <= _winattn.MAX_WINDOW)


def check_shapes(qkv, bias_table, num_heads, window_size, shift_size):
    """Shape and dtype contract; raises before anything is launched.  Works on fake tensors.  Returns
    (B, Hp, Wp, C, H, D, ws, shift, wide)."""
    ws, shift, H = int(window_size), int(shift_size), int(num_heads)
    if qkv.dim() != 4:
        raise RuntimeError("%s: qkv [B, Hp, Wp, 3C] is required, got %s" % (OP, tuple(qkv.shape)))
    B, Hp, Wp, C3 = qkv.shape
    if H < 1 or C3 < 3 or C3 % (3 * H):
        raise RuntimeError("%s: the %d channels of qkv are not divisible by 3 times %d heads" % (OP, C3, H))
    C = C3 // 3
    D = C // H
    if D % 4 or not 4 <= D <= _winattn.MAX_HEAD_DIM:
        raise RuntimeError("%s: the head dimension must be a multiple of 4 in [4, %d], got %d" % (OP, _winattn.MAX_HEAD_DIM, D))
    if not 1 <= ws <= _winattn.MAX_WINDOW:
        raise RuntimeError("%s: the window size must be in [1, %d], got %d" % (OP, _winattn.MAX_WINDOW, ws))
    if not 0 <= shift < ws:
        raise RuntimeError("%s: the shift must be in [0, window_size), got %d beside a window of %d" % (OP, shift, ws))
    if Hp % ws or Wp % ws:
        raise RuntimeError("%s: the padded map %d x %d is not a multiple of the window size %d" % (OP, Hp, Wp, ws))
    if tuple(bias_table.shape) != ((2 * ws - 1) ** 2, H):
        raise RuntimeError("%s: bias_table must be [%d, %d] for a window of %d and %d heads, got %s"
                           % (OP, (2 * ws - 1) ** 2, H, ws, H, tuple(bias_table.shape)))
    if qkv.dtype not in DTYPES:
        raise RuntimeError("%s: unsupported dtype %s (float32 / bfloat16 / float16)" % (OP, qkv.dtype))
    wide = bias_table.dtype != qkv.dtype
    if wide and bias_table.dtype != torch.float32:
        raise RuntimeError("%s: bias_table must have the dtype of qkv, or be float32 beside a 16-bit qkv, got %s beside %s"
                           % (OP, bias_table.dtype, qkv.dtype))
    if B * Hp * Wp > _MAX31:
        raise RuntimeError("%s: B * Hp * Wp must fit 31 bits" % OP)
    return B, Hp, Wp, C, H, D, ws, shift, wide


def scale_of(scale, head_dim):
    return float(head_dim) ** -0.5 if scale is None else float(scale)


def _forward(qkv, bias_table, num_heads, window_size, shift_size, scale, want_lse=True):
    """(out [B, Hp, Wp, C] in qkv's dtype, lse [B, nW, H, N] float32, out_acc); the last two are what a backward needs and are
    None unless ``want_lse``.  out_acc [B, Hp, Wp, C] float32 is ``out`` before its rounding to a 16-bit dtype, and None for
    float32 operands, whose ``out`` is that already."""
    B, Hp, Wp, C, H, D, ws, shift, wide = check_shapes(qkv, bias_table, num_heads, window_size, shift_size)
    _check_device(OP, [("qkv", qkv), ("bias_table", bias_table)])
    out = torch.empty((B, Hp, Wp, C), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B, (Hp // ws) * (Wp // ws), H, ws * ws), dtype=torch.float32, device=qkv.device) if want_lse else None
    acc = None
    if want_lse and qkv.dtype in (torch.bfloat16, torch.float16):
        acc = torch.empty((B, Hp, Wp, C), dtype=torch.float32, device=qkv.device)
    if out.numel():
        _winattn.forward(_native.dtype_code(qkv.dtype), wide, qkv.contiguous(), bias_table.contiguous(), scale_of(scale, D),
                         _winattn.Shape(B, Hp, Wp, H, D, ws, shift), out, lse, acc)
    return out, lse, acc


def _backward(grad_out, qkv, bias_table, out, lse, num_heads, window_size, shift_size, scale, wants):
    """(grad_qkv, grad_bias_table), dense and in their operand's dtype, None where ``wants`` is False.  ``out`` is the forward's
    result in float32: its out_acc for 16-bit operands.  Two launches for grad_qkv, three for grad_bias_table."""
    _require(any(wants), "%s: no gradient is asked for" % OP)
    B, Hp, Wp, C, H, D, ws, shift, wide = check_shapes(qkv, bias_table, num_heads, window_size, shift_size)
    _check_device(OP, [("grad_out", grad_out), ("qkv", qkv), ("bias_table", bias_table), ("out", out), ("lse", lse)])
    _require(grad_out.shape == out.shape and grad_out.dtype == qkv.dtype, "%s: the gradient of out must have its shape and dtype" % OP)
    empty = not out.numel()
    new = torch.zeros if empty else torch.empty
    grads = [new(t.shape, dtype=t.dtype, device=t.device) if want else None for t, want in zip((qkv, bias_table), wants)]
    if not empty:
        shape = _winattn.Shape(B, Hp, Wp, H, D, ws, shift)
        code = _native.dtype_code(qkv.dtype)
        workspace = None
        if wants[1]:
            workspace = torch.empty(_winattn.workspace_bytes(shape), dtype=torch.uint8, device=qkv.device)
        _winattn.backward(code, wide, qkv.contiguous(), bias_table.contiguous(), out.contiguous(), grad_out.contiguous(), lse,
                          scale_of(scale, D), shape, grads[0], grads[1], workspace)
    return tuple(grads)


def setup_context(ctx, inputs, output):
    qkv, bias_table, num_heads, window_size, shift_size, scale = inputs
    out, lse, acc = output
    ctx.geometry = (int(num_heads), int(window_size), int(shift_size), scale)
    ctx.mark_non_differentiable(*(t for t in (lse, acc) if t is not None))
    ctx.save_for_backward(qkv, bias_table, out if acc is None else acc, lse)


def backward(run, ctx, grad_out, grad_lse, grad_acc=None):
    """The autograd formula; ``run`` is :func:`_backward`."""
    wants = tuple(ctx.needs_input_grad[:2])
    if not any(wants):
        return (None,) * 6
    qkv, bias_table, out, lse = ctx.saved_tensors
    return run(grad_out, qkv, bias_table, out, lse, *ctx.geometry, wants) + (None,) * 4


class WindowAttentionFunction(torch.autograd.Function):
    """``window_attention`` for eager code: ``apply(qkv, bias_table, num_heads, window_size, shift_size, scale or None)`` ->
    (out, lse, out_acc or None).  Saves qkv, the table, out in float32 (out_acc for 16-bit operands) and lse -- no windows, no
    probabilities, no mask; only out is differentiable.  The backward computes the gradients autograd asks for."""
    @staticmethod
    def forward(qkv, bias_table, num_heads, window_size, shift_size, scale):
        return _forward(qkv, bias_table, num_heads, window_size, shift_size, scale)

    setup_context = staticmethod(setup_context)
    backward = eager_backward(backward, _backward)


def relative_rows(window_size, device=None):
    """[N, N] int64: the table row (iy - jy + ws - 1) * (2 ws - 1) + (ix - jx + ws - 1) of query token i and key token j."""
    ws = int(window_size)
    t = torch.arange(ws * ws, device=device)
    y, x = t // ws, t % ws
    return (y[:, None] - y[None, :] + ws - 1) * (2 * ws - 1) + (x[:, None] - x[None, :] + ws - 1)


def shift_regions(Hp, Wp, window_size, shift_size, device=None):
    """[Hp, Wp] int64: region = 3 r(ys, Hp) + r(xs, Wp) with r(c, n) = (c >= n - ws) + (c >= n - shift), at the shifted
    coordinates (ys, xs)."""
    ws, shift = int(window_size), int(shift_size)
    band = lambda n: ((torch.arange(n, device=device) >= n - ws).long() + (torch.arange(n, device=device) >= n - shift).long())   # noqa: E731
    return 3 * band(Hp)[:, None] + band(Wp)[None, :]


def composite(qkv, bias_table, num_heads, window_size, shift_size=0, scale=None):
    """The same function in torch ops (what the compiled path traces)."""
    B, Hp, Wp, C3 = qkv.shape
    H, ws, shift = int(num_heads), int(window_size), int(shift_size)
    C = C3 // 3
    D, N, ny, nx = C // H, ws * ws, Hp // ws, Wp // ws
    x = torch.roll(qkv, (-shift, -shift), (1, 2)) if shift else qkv
    q, k, v = x.reshape(B, ny, ws, nx, ws, 3, H, D).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, B, ny * nx, H, N, D).unbind(0)
    logits = torch.matmul(q * scale_of(scale, D), k.transpose(-1, -2))
    bias = bias_table[relative_rows(ws, qkv.device).reshape(-1)].reshape(N, N, H).permute(2, 0, 1)
    logits = logits + bias.to(logits.dtype)
    if shift:
        region = shift_regions(Hp, Wp, ws, shift, qkv.device).reshape(ny, ws, nx, ws).permute(0, 2, 1, 3).reshape(ny * nx, N)
        differ = region[:, :, None] != region[:, None, :]
        logits = logits + (differ.to(logits.dtype) * MASKED)[:, None]
    out = torch.matmul(torch.softmax(logits, -1), v)
    out = out.reshape(B, ny, nx, H, ws, ws, D).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, Hp, Wp, C)
    return torch.roll(out, (shift, shift), (1, 2)) if shift else out


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def window_attention(qkv, bias_table, num_heads, window_size, shift_size=0, scale=None):
    """A Swin block's (shifted-)window attention between its ``qkv`` and ``proj`` Linears as one HIP kernel pass
    (include/winattn.h): ``qkv [B, Hp, Wp, 3C]`` -- the ``qkv`` Linear on the padded, un-rolled, un-partitioned map, channels in
    the order of ``reshape(..., 3, num_heads, D)`` -- and ``bias_table [(2 ws - 1)^2, num_heads]`` -> ``out [B, Hp, Wp, C]`` in
    map order, rolled back.  ``Hp`` and ``Wp`` are multiples of ``window_size`` (at most 16), ``0 <= shift_size < window_size``,
    ``D % 4 == 0`` and ``4 <= D <= 64``; ``scale`` defaults to ``D ** -0.5``.

    Token ``i = iy * ws + ix`` of window ``(wy, wx)`` sits at the shifted coordinates ``(ys, xs) = (wy * ws + iy, wx * ws + ix)``
    and reads and writes map pixel ``((ys + shift) mod Hp, (xs + shift) mod Wp)``.  ``S[i, j] = scale * (q_i . k_j) +
    table[(iy - jy + ws - 1) * (2 ws - 1) + (ix - jx + ws - 1), h] + mask(i, j)``; with a shift, ``mask`` is -100 where
    ``region(i) != region(j)``, ``region = 3 r(ys, Hp) + r(xs, Wp)``, ``r(c, n) = (c >= n - ws) + (c >= n - shift)``.
    ``out_i = sum_j softmax_j(S)[i, j] v_j``.  There is no attention dropout.

    One dtype of float32 / bfloat16 / float16 for ``qkv``; the table has the same dtype or is float32 beside a 16-bit ``qkv``
    (autocast).  Arithmetic is float32, ``out`` is rounded once.  Differentiable in ``qkv`` and ``bias_table`` (once); only the
    gradients autograd asks for are computed.  While ``torch.compiler.is_compiling()`` this is the torch composite."""
    if torch.compiler.is_compiling():
        check_shapes(qkv, bias_table, num_heads, window_size, shift_size)
        return composite(qkv, bias_table, num_heads, window_size, shift_size, scale)
    if _wants_grad(qkv, bias_table):
        return WindowAttentionFunction.apply(qkv, bias_table, num_heads, window_size, shift_size, scale)[0]
    return _forward(qkv, bias_table, num_heads, window_size, shift_size, scale, want_lse=False)[0]
