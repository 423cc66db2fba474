"""The reference's transformer layers on the fused glue operators: ``forward`` and ``forward_ffn`` of
``DeformableTransformerEncoderLayer`` and ``DeformableTransformerDecoderLayer`` (``src/models/deformable_transformer.py``) with
every ``x = norm(x + dropout(y))`` as one :func:`devis_amd.add_layer_norm` call and the FFN as
``linear2(relu_dropout(linear1(x)))``.  Signatures and call order are the reference's; ``with_pos_embed`` stays on torch and the
attention modules, ``nn.MultiheadAttention`` included, are called as they are.  No module is replaced, so state dicts are
untouched.  :func:`devis_amd.patch_transformer_layers` installs these functions on the reference's classes.

Dropout: ``p`` is the Dropout module's ``p`` in training mode, else 0.  A training call with any ``p > 0`` draws the seeds of all
of its sites with ONE ``torch.randint`` over the int64 range on the device -- one tiny launch, reproducible under
``torch.manual_seed``, safe inside a HIP-graph capture, no host read.

The replaced methods run instead -- the model then computes exactly what it computed before the patch -- when the model is
compiling (``torch.compiler.is_compiling()``), the tensors are on the CPU, ``self.activation`` is not ``F.relu``, a norm is not
an affine ``LayerNorm`` over the last dimension, there are more than 1024 channels, or the dtypes are not ones the kernels take.
Each of the two methods decides for itself (the replaced ``forward`` calls ``self.forward_ffn``, which may still be fused).
A norm site whose ``delta`` comes back from its attention module in a dtype the kernels do not take beside ``x``'s computes
the reference's expression for that site.
"""
import torch
import torch.nn.functional as F

from .. import _addnorm
from ..functions import add_norm

STOCK = "_devis_amd_stock_layer"        # on a patched class: {"forward": ..., "forward_ffn": ...}, what the patch replaced
_INT64_MIN, _INT64_MAX = -(1 << 63), (1 << 63) - 1


def _stock(self, name):
    """The replaced function ``name`` of the layer's class (called with ``self`` first)."""
    return getattr(type(self), STOCK)[name]


def _norm_ok(norm, x):
    return (isinstance(norm, torch.nn.LayerNorm) and norm.weight is not None and norm.bias is not None and
            tuple(norm.normalized_shape) == (x.shape[-1],) and norm.weight.dtype == norm.bias.dtype and
            add_norm.supported(x.dtype, x.dtype, norm.weight.dtype))


def _on_gpu(x):
    return x.is_cuda


def _fusable(self, x, norms):
    """Whether this call takes the fused route (the module's docstring lists what sends it to the replaced methods)."""
    if torch.compiler.is_compiling() or not isinstance(x, torch.Tensor) or not _on_gpu(x) or x.dim() < 1:
        return False
    if self.activation is not F.relu or not 1 <= x.shape[-1] <= _addnorm.MAX_CHANNELS:
        return False
    return all(_norm_ok(norm, x) for norm in norms)


def _seeds(self, x, dropouts):
    """One int64 seed per dropout site of the call ([n] on x's device), or None when none of them drops."""
    if not self.training or not any(d.p > 0 for d in dropouts):
        return None
    return torch.randint(_INT64_MIN, _INT64_MAX, (len(dropouts),), dtype=torch.int64, device=x.device)


def _p(self, dropout):
    return dropout.p if self.training else 0.0


def _seed(seeds, i):
    return None if seeds is None else seeds[i:i + 1]


def _site(self, x, delta, dropout, norm, seed):
    """One norm site: ``norm(x + dropout(delta))``."""
    if delta.shape != x.shape or not add_norm.supported(x.dtype, delta.dtype, norm.weight.dtype):
        return norm(x + dropout(delta))
    p = _p(self, dropout)
    return add_norm.add_layer_norm(x, delta, norm.weight, norm.bias, norm.eps, p=p, seed=seed if p > 0 else None)


def _ffn(self, x, inner_dropout, outer_dropout, norm, seeds, at):
    """The FFN with the seeds ``at`` and ``at + 1`` of the call."""
    p = _p(self, inner_dropout)
    hidden = self.linear1(x)
    if hidden.dtype in add_norm.DTYPES:
        hidden = add_norm.relu_dropout(hidden, p=p, seed=_seed(seeds, at) if p > 0 else None)
    else:
        hidden = inner_dropout(self.activation(hidden))
    return _site(self, x, self.linear2(hidden), outer_dropout, norm, _seed(seeds, at + 1))


# ---- DeformableTransformerEncoderLayer ------------------------------------------------------------------------------------

def encoder_forward_ffn(self, src):
    if not _fusable(self, src, (self.norm2,)):
        return _stock(self, "forward_ffn")(self, src)
    seeds = _seeds(self, src, (self.dropout2, self.dropout3))
    return _ffn(self, src, self.dropout2, self.dropout3, self.norm2, seeds, 0)


def encoder_forward(self, src, pos, reference_points, spatial_shapes, level_start_index, **kwargs):
    if not _fusable(self, src, (self.norm1, self.norm2)):
        return _stock(self, "forward")(self, src, pos, reference_points, spatial_shapes, level_start_index, **kwargs)
    seeds = _seeds(self, src, (self.dropout1, self.dropout2, self.dropout3))
    # self attention
    src2, *_ = self.self_attn(self.with_pos_embed(src, pos), reference_points, src, spatial_shapes, level_start_index, **kwargs)
    src = _site(self, src, src2, self.dropout1, self.norm1, _seed(seeds, 0))
    # ffn
    if type(self).forward_ffn is not encoder_forward_ffn:      # (a subclass with an FFN of its own)
        return self.forward_ffn(src)
    return _ffn(self, src, self.dropout2, self.dropout3, self.norm2, seeds, 1)


# ---- DeformableTransformerDecoderLayer ------------------------------------------------------------------------------------

def decoder_forward_ffn(self, tgt):
    if not _fusable(self, tgt, (self.norm3,)):
        return _stock(self, "forward_ffn")(self, tgt)
    seeds = _seeds(self, tgt, (self.dropout3, self.dropout4))
    return _ffn(self, tgt, self.dropout3, self.dropout4, self.norm3, seeds, 0)


def decoder_forward(self, tgt, query_pos, reference_points, src, src_spatial_shapes, level_start_index, **kwargs):
    if not _fusable(self, tgt, (self.norm1, self.norm2, self.norm3)):
        return _stock(self, "forward")(self, tgt, query_pos, reference_points, src, src_spatial_shapes, level_start_index, **kwargs)
    seeds = _seeds(self, tgt, (self.dropout2, self.dropout1, self.dropout3, self.dropout4))
    # self attention
    q = k = self.with_pos_embed(tgt, query_pos)
    tgt2 = self.self_attn(q.transpose(0, 1), k.transpose(0, 1), tgt.transpose(0, 1))[0].transpose(0, 1)
    tgt = _site(self, tgt, tgt2, self.dropout2, self.norm2, _seed(seeds, 0))
    # cross attention
    tgt2, *_ = self.cross_attn(self.with_pos_embed(tgt, query_pos), reference_points, src, src_spatial_shapes, level_start_index,
                               **kwargs)
    tgt = _site(self, tgt, tgt2, self.dropout1, self.norm1, _seed(seeds, 1))
    # ffn
    if type(self).forward_ffn is not decoder_forward_ffn:
        return self.forward_ffn(tgt)
    return _ffn(self, tgt, self.dropout3, self.dropout4, self.norm3, seeds, 2)


METHODS = (("DeformableTransformerEncoderLayer", "forward", encoder_forward),
           ("DeformableTransformerEncoderLayer", "forward_ffn", encoder_forward_ffn),
           ("DeformableTransformerDecoderLayer", "forward", decoder_forward),
           ("DeformableTransformerDecoderLayer", "forward_ffn", decoder_forward_ffn))


def patch(module):
    """Installs the four methods on the two classes of ``module``; returns what they replaced."""
    classes = {name: getattr(module, name) for name, _, _ in METHODS}
    previous = {}
    for cls_name, name, ours in METHODS:
        cls = classes[cls_name]
        current = getattr(cls, name)
        if current is ours:                                  # (patched twice: the stock methods are the recorded ones)
            current = getattr(cls, STOCK)[name]
        previous[(cls_name, name)] = current
    for cls_name, name, ours in METHODS:
        cls = classes[cls_name]
        stock = dict(cls.__dict__.get(STOCK, {}))
        stock[name] = previous[(cls_name, name)]
        setattr(cls, STOCK, stock)
        setattr(cls, name, ours)
    return previous


def unpatch(module, previous):
    """Puts back what :func:`patch` returned."""
    for (cls_name, name), method in previous.items():
        cls = getattr(module, cls_name)
        setattr(cls, name, method)
        if STOCK in cls.__dict__:
            delattr(cls, STOCK)
