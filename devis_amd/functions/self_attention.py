"""Host side of the decoder's query self-attention (include/selfattn.h):
``multihead_attention(q, k, v, num_heads)`` = ``dropout(softmax(q_h k_h^T / sqrt(D))) v_h`` per batch entry and head -- what
``nn.MultiheadAttention`` computes between its input projections and ``out_proj`` --, one kernel pass forward and at most two
backward.  Argument checks, the output tensors, the kernel launches and the autograd Function.

``q``, ``k`` and ``v`` are handed to the kernels as the views they are (any strides with a last stride of 1), so the two column
halves of one ``[L, N, 2E]`` projection and ``batch_first`` tensors need no copy.  No probability matrix and no mask is stored:
the Function saves the operands, ``out`` in float32 (for 16-bit operands a copy the forward writes before it rounds: the
backward's ``delta = sum(dO * O)`` cancels against ``dP`` and needs the unrounded rows), one float32 per row (``lse``) and the
seed, and the backward recomputes the rest.

The dropout mask is a function of ``(seed, n, h, i, j)`` (Philox4x32-10; the rule is in the header).  ``seed`` is an int64
DEVICE tensor of one element that only the kernels read -- nothing here reads a device value on the host, and a HIP graph
replayed after ``seed.copy_(...)`` draws a new mask.  Every sum has a fixed order and there are no atomics: every result is
bitwise reproducible and nothing here raises or warns under ``torch.use_deterministic_algorithms(True)``.

This is NOT a ``torch.library`` op.  While ``torch.compiler.is_compiling()`` is true the public function computes the torch
composite -- ``bmm``, ``softmax``, ``F.dropout``, ``bmm`` --, whose mask then comes from torch's generator and IGNORES ``seed``.
Compiled and exported models neither break a graph nor change.

There is no CPU path and no eager fallback: CPU tensors raise, a failing kernel call raises.
"""
import math

import torch
import torch.nn.functional as F

from .. import _native, _selfattn
from ._common import _check_device, _require, eager_backward
from .add_norm import check_p

OP = "multihead_attention"
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_MAX31 = (1 << 31) - 1


def supported(dtype, head_dim):
    """Whether the kernels take this storage dtype and this many channels per head (include/selfattn.h)."""
    return dtype in DTYPES and head_dim % 4 == 0 and 4 <= head_dim <= _selfattn.MAX_HEAD_DIM


def check_shapes(q, k, v, num_heads):
    """Shape and dtype contract; raises before anything is launched.  Works on fake tensors.  Returns (L, S, N, E, H, D)."""
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
        raise RuntimeError("%s: q [L, N, E], k and v [S, N, E] are required, got %s, %s and %s"
                           % (OP, tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    L, N, E = q.shape
    S = k.shape[0]
    if k.shape != v.shape or tuple(k.shape[1:]) != (N, E):
        raise RuntimeError("%s: k and v must be [S, %d, %d] beside q %s, got %s and %s"
                           % (OP, N, E, tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    H = int(num_heads)
    if H < 1 or E < 1 or E % H:
        raise RuntimeError("%s: %d channels are not divisible by %d heads" % (OP, E, H))
    D = E // H
    if D % 4 or not 4 <= D <= _selfattn.MAX_HEAD_DIM:
        raise RuntimeError("%s: the head dimension must be a multiple of 4 in [4, %d], got %d" % (OP, _selfattn.MAX_HEAD_DIM, D))
    if not (q.dtype == k.dtype == v.dtype):
        raise RuntimeError("%s: q, k and v must have one dtype, got %s, %s and %s" % (OP, q.dtype, k.dtype, v.dtype))
    if q.dtype not in DTYPES:
        raise RuntimeError("%s: unsupported dtype %s (float32 / bfloat16 / float16)" % (OP, q.dtype))
    if max(L, S, N, E) > _MAX31:
        raise RuntimeError("%s: L, S, N and E must fit 31 bits" % OP)
    return L, S, N, E, H, D


def as_view(t):
    """``t`` as the kernels take it: itself when its last stride is 1 and its strides fit 31 bits, else a dense copy."""
    strides = t.stride()
    if (strides[2] == 1 or t.shape[2] == 1) and 0 <= strides[0] <= _MAX31 and 0 <= strides[1] <= _MAX31:
        return t if strides[2] == 1 else t.as_strided(t.shape, (strides[0], strides[1], 1))
    return t.contiguous()


def _forward(q, k, v, seed, num_heads, p, want_lse=True):
    """(out [L, N, E] in q's dtype, lse [N * H, L] float32, out_acc); the last two are what a backward needs and are None
    unless ``want_lse``.  out_acc [L, N, E] float32 is ``out`` before its rounding to a 16-bit dtype, and None for float32
    operands, whose ``out`` is that already."""
    p = check_p(OP, p, seed)
    L, S, N, E, H, D = check_shapes(q, k, v, num_heads)
    seed = seed if p > 0.0 else None
    _check_device(OP, [("q", q), ("k", k), ("v", v), ("seed", seed)])
    new = torch.empty if S else torch.zeros
    out = new((L, N, E), dtype=q.dtype, device=q.device)
    lse = torch.empty((N * H, L), dtype=torch.float32, device=q.device) if want_lse else None
    acc = new((L, N, E), dtype=torch.float32, device=q.device) if want_lse and q.dtype in (torch.bfloat16, torch.float16) else None
    if L and N and S:
        extra = () if acc is None else (acc,)            # (float32: the call the binding has always taken)
        _selfattn.forward(_native.dtype_code(q.dtype), as_view(q), as_view(k), as_view(v), seed, p,
                          _selfattn.Shape(L, S, N, E, H), out, lse, *extra)
    return out, lse, acc


def _backward(grad_out, q, k, v, out, lse, seed, num_heads, p, wants):
    """(grad_q, grad_k, grad_v), dense and in their operand's dtype, None where ``wants`` is False.  ``out`` is the forward's
    result in float32: its out_acc for 16-bit operands.  One launch for grad_q, one for grad_k and / or grad_v."""
    _require(any(wants), "%s: no gradient is asked for" % OP)
    L, S, N, E, H, D = check_shapes(q, k, v, num_heads)
    seed = seed if p > 0.0 else None
    _check_device(OP, [("grad_out", grad_out), ("q", q), ("k", k), ("v", v), ("out", out), ("lse", lse), ("seed", seed)])
    _require(grad_out.shape == out.shape and grad_out.dtype == q.dtype, "%s: the gradient of out must have its shape and dtype" % OP)
    empty = not (L and N and S)
    new = torch.zeros if empty else torch.empty
    grads = [new(t.shape, dtype=t.dtype, device=t.device) if want else None for t, want in zip((q, k, v), wants)]
    if not empty:
        _selfattn.backward(_native.dtype_code(q.dtype), as_view(q), as_view(k), as_view(v), out.contiguous(),
                           grad_out.contiguous(), lse, seed, p, _selfattn.Shape(L, S, N, E, H), *grads)
    return tuple(grads)


def setup_context(ctx, inputs, output):
    q, k, v, seed, num_heads, p = inputs
    out, lse, acc = output
    ctx.p, ctx.num_heads = float(p), int(num_heads)
    ctx.mark_non_differentiable(*(t for t in (lse, acc) if t is not None))
    ctx.save_for_backward(q, k, v, out if acc is None else acc, lse, seed if ctx.p > 0.0 else None)


def backward(run, ctx, grad_out, grad_lse, grad_acc=None):
    """The autograd formula; ``run`` is :func:`_backward`."""
    wants = tuple(ctx.needs_input_grad[:3])
    if not any(wants):
        return (None,) * 6
    q, k, v, out, lse, seed = ctx.saved_tensors
    return run(grad_out, q, k, v, out, lse, seed, ctx.num_heads, ctx.p, wants) + (None,) * 3


class MultiheadAttentionFunction(torch.autograd.Function):
    """``multihead_attention`` for eager code: ``apply(q, k, v, seed or None, num_heads, p)`` -> (out, lse, out_acc or None).
    Saves the operand views, out in float32 (out_acc for 16-bit operands), lse and the seed -- no probabilities, no mask; only
    out is differentiable.  The backward computes the gradients autograd asks for and launches nothing when it asks for none."""
    @staticmethod
    def forward(q, k, v, seed, num_heads, p):
        return _forward(q, k, v, seed, num_heads, p)

    setup_context = staticmethod(setup_context)
    backward = eager_backward(backward, _backward)


def composite(q, k, v, num_heads, p=0.0):
    """The same function in torch ops (what the compiled path traces): the mask comes from torch's generator."""
    L, N, E = q.shape
    S, H = k.shape[0], int(num_heads)
    D = E // H
    heads = lambda t, rows: t.reshape(rows, N * H, D).transpose(0, 1)      # noqa: E731
    logits = torch.bmm(heads(q, L), heads(k, S).transpose(1, 2)) / math.sqrt(D)
    prob = torch.softmax(logits, -1)
    if p > 0.0:
        prob = F.dropout(prob, p, True)
    return torch.bmm(prob, heads(v, S)).transpose(0, 1).reshape(L, N, E)


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def multihead_attention(q, k, v, num_heads, *, p=0.0, seed=None):
    """``dropout_p(softmax(q_h k_h^T / sqrt(D))) v_h`` for every batch entry and head as one HIP kernel pass
    (include/selfattn.h): ``q [L, N, E]``, ``k`` and ``v [S, N, E]`` -> ``out [L, N, E]``, head ``h`` over the channels
    ``h * D .. h * D + D - 1`` with ``D = E / num_heads``, ``D % 4 == 0`` and ``4 <= D <= 64``.  One dtype of float32 / bfloat16 /
    float16; arithmetic is float32, ``out`` is rounded once.  The operands may be any views whose last stride is 1 (column halves
    of a wider projection, ``batch_first`` transposes); other views are made dense first.  ``S == 0`` gives zeros.

    ``p`` is the probability of dropping a probability (the caller passes 0 in eval mode); ``seed``, an int64 device tensor of
    one element, is required when ``p > 0`` (ValueError otherwise), read by the kernels only, and ignored when ``p == 0``.  The
    mask is a function of (seed, n, h, i, j): the backward recomputes it, and a graph replay after ``seed.copy_`` draws a new one.

    Differentiable in q, k and v (once); the gradients are dense.  While ``torch.compiler.is_compiling()`` this is the torch
    composite: its mask comes from torch's generator and ``seed`` is ignored."""
    if torch.compiler.is_compiling():
        p = check_p(OP, p, seed)
        check_shapes(q, k, v, num_heads)
        return composite(q, k, v, num_heads, p)
    if _wants_grad(q, k, v):
        return MultiheadAttentionFunction.apply(q, k, v, seed, num_heads, p)[0]
    return _forward(q, k, v, seed, num_heads, p, want_lse=False)[0]
