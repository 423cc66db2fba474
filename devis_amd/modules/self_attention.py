"""``nn.MultiheadAttention`` on the fused attention operator: :class:`FusedMultiheadAttention` is a
subclass with the same constructor, parameter names and ``forward`` signature -- it loads the reference's state dict -- whose
``forward`` is two or three ``F.linear`` calls, :func:`devis_amd.multihead_attention` and ``out_proj``.
:func:`devis_amd.patch_self_attention` turns the ``nn.MultiheadAttention`` modules of a model into it by setting ``__class__``:
no module is replaced, state dicts are untouched, ``copy.deepcopy`` keeps the class.

The fused route runs when the tensors are 3-D and on the GPU, the model is not compiling
(``torch.compiler.is_compiling()``), ``_qkv_same_embed_dim`` is true, there is no ``bias_k`` / ``bias_v`` and no
``add_zero_attn``, no ``attn_mask``, no ``key_padding_mask`` and no ``is_causal``, ``key.shape == value.shape``, the dtype the
projections return and the head dimension are ones the kernels take (float32 / bfloat16 / float16; a multiple of 4 up to 64),
and ``need_weights`` is false or the module's ``discard_attention_weights`` is true.  Every other call runs
``nn.MultiheadAttention.forward`` unchanged.

On the fused route a call with ``query is key`` -- or with two equal views of one tensor, the decoder layer's
``self_attn(q.transpose(0, 1), k.transpose(0, 1), ...)`` with ``q is k`` -- projects both with ONE ``F.linear`` on
``in_proj_weight[:2E]`` and hands the two column halves of the result to the operator as views;
``value`` is one more ``F.linear``.  It returns ``(out, None)``: with ``discard_attention_weights`` and ``need_weights=True``
that ``None`` stands where torch returns the head-averaged weights, which the reference throws away (``[0]``).

Dropout: ``p`` is the module's ``dropout`` in training mode, else 0.  A training call with ``p > 0`` draws its seed with one
one-element ``torch.randint`` over the int64 range on the device -- reproducible under ``torch.manual_seed``, safe inside a
HIP-graph capture, no host read.  Under autocast the projections return 16-bit tensors and the operator takes them.
"""
import torch
import torch.nn.functional as F
from torch import nn

from ..functions import self_attention

_INT64_MIN, _INT64_MAX = -(1 << 63), (1 << 63) - 1
FLAG = "discard_attention_weights"


def _on_gpu(x):
    return x.is_cuda


def _projected_dtype(module, query):
    """The dtype ``F.linear(query, module.in_proj_weight)`` returns."""
    if torch.is_autocast_enabled(query.device.type):
        return torch.get_autocast_dtype(query.device.type)
    return module.in_proj_weight.dtype


def _same_tensor(a, b):
    """``a is b``, or both are the same view (shape, strides, offset) of one base tensor."""
    if a is b:
        return True
    return (a._base is not None and a._base is b._base and a.shape == b.shape and a.stride() == b.stride() and
            a.storage_offset() == b.storage_offset() and a.dtype == b.dtype)


class FusedMultiheadAttention(nn.MultiheadAttention):
    """``nn.MultiheadAttention`` whose attention between the projections is one HIP kernel pass (the module's docstring lists
    when; otherwise the stock forward runs)."""
    discard_attention_weights = False

    def _fusable(self, query, key, value, key_padding_mask, need_weights, attn_mask, is_causal):
        if torch.compiler.is_compiling() or not all(isinstance(t, torch.Tensor) for t in (query, key, value)):
            return False
        if query.dim() != 3 or key.dim() != 3 or key.shape != value.shape or not all(_on_gpu(t) for t in (query, key, value)):
            return False
        if need_weights and not self.discard_attention_weights:
            return False
        if key_padding_mask is not None or attn_mask is not None or is_causal:
            return False
        if not self._qkv_same_embed_dim or self.bias_k is not None or self.bias_v is not None or self.add_zero_attn:
            return False
        batch = 0 if self.batch_first else 1
        if query.shape[2] != self.embed_dim or key.shape[2] != self.embed_dim or query.shape[batch] != key.shape[batch]:
            return False                                     # (the stock forward raises)
        if not (query.dtype == key.dtype == value.dtype):
            return False
        return self_attention.supported(_projected_dtype(self, query), self.head_dim)

    def forward(self, query, key, value, key_padding_mask=None, need_weights=True, attn_mask=None, average_attn_weights=True,
                is_causal=False):
        if not self._fusable(query, key, value, key_padding_mask, need_weights, attn_mask, is_causal):
            return super().forward(query, key, value, key_padding_mask=key_padding_mask, need_weights=need_weights,
                                   attn_mask=attn_mask, average_attn_weights=average_attn_weights, is_causal=is_causal)
        E, weight, bias = self.embed_dim, self.in_proj_weight, self.in_proj_bias
        part = lambda lo, hi: None if bias is None else bias[lo:hi]      # noqa: E731
        if _same_tensor(query, key):
            qk = F.linear(query, weight[:2 * E], part(0, 2 * E))
            q, k = qk[..., :E], qk[..., E:]
        else:
            q, k = F.linear(query, weight[:E], part(0, E)), F.linear(key, weight[E:2 * E], part(E, 2 * E))
        v = F.linear(value, weight[2 * E:], part(2 * E, 3 * E))
        if self.batch_first:
            q, k, v = q.transpose(0, 1), k.transpose(0, 1), v.transpose(0, 1)
        p = self.dropout if self.training else 0.0
        seed = None
        if p > 0.0:
            seed = torch.randint(_INT64_MIN, _INT64_MAX, (1,), dtype=torch.int64, device=query.device)
        out = self_attention.multihead_attention(q, k, v, self.num_heads, p=p, seed=seed)
        out = self.out_proj(out)
        return (out.transpose(0, 1) if self.batch_first else out), None


def patch(root_module, discard_weights=True):
    """Every module under ``root_module`` whose type is exactly ``nn.MultiheadAttention`` becomes a
    :class:`FusedMultiheadAttention` with ``discard_attention_weights = discard_weights``; returns what :func:`unpatch` needs."""
    previous = []
    for module in root_module.modules():
        if type(module) is nn.MultiheadAttention:
            previous.append((module, nn.MultiheadAttention))
            module.__class__ = FusedMultiheadAttention
            setattr(module, FLAG, bool(discard_weights))
    return previous


def unpatch(previous):
    """Puts back what :func:`patch` returned."""
    for module, cls in previous:
        module.__class__ = cls
        module.__dict__.pop(FLAG, None)
