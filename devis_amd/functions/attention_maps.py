"""Host side of the mask head's attention maps (include/attmap.h): argument checks, the output and
workspace tensors, the two kernel passes, and in the backward the two batched GEMMs (``torch`` -> rocBLAS) over the ``dl``
buffer the softmax-gradient kernel writes.  The custom ops of :mod:`devis_amd.ops` run exactly this code.

Every sum has a fixed order -- there are no float atomics -- so ``out`` and both gradients are bitwise reproducible and
nothing here raises or warns under ``torch.use_deterministic_algorithms(True)``.

There is no CPU path and no eager fallback: CPU tensors raise, a failing kernel call raises.
"""
import torch

from .. import _attmap, _native
from ._common import _check_device, _require, _workspace, eager_backward

NEED_Q, NEED_K = _attmap.GRAD_Q, _attmap.GRAD_K
NEED_ALL = NEED_Q | NEED_K


def grads_mask(need_q, need_k):
    """``ctx.needs_input_grad`` flags -> the `grads` mask of the backward op."""
    return (NEED_Q if need_q else 0) | (NEED_K if need_k else 0)


def default_scale(q, num_heads):
    return float(q.shape[-1] // num_heads) ** -0.5


def check_shapes(q, k, mask, num_heads, out_dtype=None):
    """Shape and dtype contract of attention_maps; raises before anything is launched.  Works on fake tensors.  Returns
    (B, Q, n, c, H, W, out's dtype)."""
    _require(q.dim() == 3 and k.dim() == 4, "attention_maps: q must be [B, Q, n*c] and k [B, n*c, H, W]")
    B, Q, D = q.shape
    _require(isinstance(num_heads, int) and num_heads > 0, "attention_maps: num_heads must be a positive int")
    _require(D > 0 and D % num_heads == 0, "attention_maps: %s channels are not a multiple of the %d heads" % (D, num_heads))
    _require(k.shape[0] == B and k.shape[1] == D, "attention_maps: k must be [B, n*c, H, W] = [%s, %s, H, W], got %s"
             % (B, D, tuple(k.shape)))
    H, W = k.shape[2], k.shape[3]
    _require(H > 0 and W > 0, "attention_maps: the map would be empty (%s x %s)" % (H, W))
    _require(k.dtype == q.dtype, "attention_maps: k must have q's dtype")
    _native.dtype_code(q.dtype)         # raises on an unsupported dtype
    if mask is not None:
        _require(mask.dim() == 3 and mask.shape[0] == B and mask.shape[1] == H and mask.shape[2] == W,
                 "attention_maps: mask must be [B, H, W] = [%s, %s, %s], got %s" % (B, H, W, tuple(mask.shape)))
        _require(mask.dtype in (torch.bool, torch.uint8), "attention_maps: mask must be a bool (or uint8) tensor")
    return B, Q, num_heads, D // num_heads, H, W, _attmap.out_dtype(q.dtype, out_dtype)


def _forward(q, k, mask, num_heads, scale, out_dtype=None):
    """out [B, Q, n, H, W]: two kernel passes, no logits tensor."""
    _check_device("attention_maps", [("q", q), ("k", k), ("mask", mask)])
    B, Q, n, c, H, W, odt = check_shapes(q, k, mask, num_heads, out_dtype)
    out = torch.empty((B, Q, n, H, W), dtype=odt, device=q.device)
    if B == 0 or Q == 0:
        return out
    shape = _attmap.Shape(B, Q, n, c, H, W)
    code, out_code = _native.dtype_code(q.dtype), _native.dtype_code(odt)
    if mask is not None:
        mask = mask.contiguous()
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    _attmap.forward(code, out_code, q.contiguous(), k.contiguous(), mask, shape, scale, _workspace(_attmap, code, shape, q.device), out)
    return out


def _backward(grad_out, q, k, out, num_heads, scale, grads=NEED_ALL):
    """(grad_q, grad_k) for the gradients in ``grads``; the other is neither allocated nor computed and comes back None.
    Both are contractions of the same ``dl``, so each alone has the bits it has in a full backward."""
    _require(0 <= grads <= NEED_ALL, "attention_maps: grads must be a mask of NEED_Q and NEED_K")
    _check_device("attention_maps", [("q", q), ("k", k), ("out", out), ("grad_out", grad_out)])
    B, Q, n, c, H, W, _ = check_shapes(q, k, None, num_heads)
    odt = _attmap.out_dtype(q.dtype, out.dtype)
    _require(tuple(out.shape) == (B, Q, n, H, W), "attention_maps: out must be [B, Q, n, H, W]")
    _require(tuple(grad_out.shape) == (B, Q, n, H, W) and grad_out.dtype == odt,
             "attention_maps: grad_out must be [B, Q, n, H, W] in out's dtype")
    if grads == 0:
        return None, None
    grad_q = grad_k = None
    if B == 0 or Q == 0:
        return (torch.zeros_like(q, memory_format=torch.contiguous_format) if grads & NEED_Q else None,
                torch.zeros_like(k, memory_format=torch.contiguous_format) if grads & NEED_K else None)
    P = H * W
    shape = _attmap.Shape(B, Q, n, c, H, W)
    code, out_code = _native.dtype_code(q.dtype), _native.dtype_code(odt)
    dl = torch.empty((B, n, Q, P), dtype=q.dtype, device=q.device)
    _attmap.backward(grads, code, out_code, out.contiguous(), grad_out.contiguous(), shape, scale,
                     _workspace(_attmap, code, shape, q.device), dl)
    if grads & NEED_Q:      # [B, n, Q, P] x [B, n, P, c] -> [B, n, Q, c]
        gq = torch.matmul(dl, k.contiguous().view(B, n, c, P).transpose(2, 3))
        grad_q = gq.permute(0, 2, 1, 3).reshape(B, Q, n * c)
    if grads & NEED_K:      # [B, n, c, Q] x [B, n, Q, P] -> [B, n, c, P]: k's own layout
        grad_k = torch.matmul(q.contiguous().view(B, Q, n, c).permute(0, 2, 3, 1), dl).view(B, n * c, H, W)
    return grad_q, grad_k


def setup_context(ctx, inputs, output):
    q, k, mask, num_heads, scale = inputs[:5]
    ctx.num_heads, ctx.scale = num_heads, scale
    ctx.save_for_backward(q, k, output)


def backward(run, ctx, grad_out):
    """The autograd formula; ``run`` is :func:`_backward`, or the backward op with its empty gradients mapped to None."""
    q, k, out = ctx.saved_tensors
    grads = grads_mask(ctx.needs_input_grad[0], ctx.needs_input_grad[1])
    grad_q, grad_k = run(grad_out, q, k, out, ctx.num_heads, ctx.scale, grads)
    return grad_q, grad_k, None, None, None, None


class AttentionMapsFunction(torch.autograd.Function):
    """``attention_maps`` for eager code: ``apply(q, k, mask, num_heads, scale, out_dtype)``.  The backward computes the
    gradients ``ctx.needs_input_grad`` names and no others."""
    forward = staticmethod(_forward)
    setup_context = staticmethod(setup_context)
    backward = eager_backward(backward, _backward)
