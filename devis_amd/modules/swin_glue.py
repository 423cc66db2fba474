"""The reference's Swin stage (``src/models/swin_backbone.py``) on the fused glue kernels, on top of the
fused window attention of :mod:`devis_amd.modules.window_attention`.  :func:`devis_amd.patch_swin_glue` installs three forwards
on the reference's classes, by name; no module is replaced, so state dicts are untouched.

``SwinTransformerBlock.forward(x, mask_matrix)`` -- :func:`block_forward`::

    (_, y)  = residual_layer_norm(x, None, norm1.., map_size=(H, W, Hp, Wp))     # norm1 and F.pad: one pass
    a       = proj_drop(proj(window_attention(qkv(y), ...)[:, :H, :W].reshape(B, H * W, C)))
    (s, y2) = residual_layer_norm(x, a, norm2.., keep=k1)                        # shortcut + drop_path, norm2: one pass
    return s + k2 * mlp(y2)

``mask_matrix`` is accepted and not read.  Under autocast ``y`` and ``y2`` are written in the autocast dtype beside the float32
stream, so the Linears that read them cast nothing.  In training, with a ``drop_path`` that is not ``nn.Identity``, the scale
vectors are the block's own module's draws, ``self.drop_path(x.new_ones(B, 1, 1)).view(B)`` -- right for any DropPath
implementation and rate, taken where the stock forward takes them, so the same seed gives the same masks; otherwise there is
no ``keep``.

``BasicLayer.forward(x, H, W)`` -- :func:`layer_forward`: when every block takes the fused route the shift mask is not built
(the attention kernels derive it) and the blocks are chained on the deferred state ``(x, delta, keep)``: a block's last add is
not executed but becomes the residual form of the next block's first call, which writes the stream and the next ``norm1`` map in
one pass.  After the last block the state is resolved once by torch.  Under ``use_checkpoint`` each block is called through
``checkpoint`` in its self-contained form.  The return tuple is the reference's.

``PatchMerging.forward(x, H, W)`` -- :func:`merge_forward`: ``reduction(patch_merge_norm(x, H, W, norm..))``.

The forward that was installed before the patch runs instead -- the module then computes exactly what it computed before --
where :func:`devis_amd.modules.window_attention._fusable` says no (compiling, CPU, float64, attention dropout in training, an
unsupported window or head dimension), where a norm is not an affine ``nn.LayerNorm`` over the channels, and above
``PRENORM_MAX_CHANNELS`` channels; a layer does so if any of its blocks does.
"""
import torch
import torch.utils.checkpoint as checkpoint
from torch import nn

from .. import _prenorm
from ..functions import pre_norm as P
from ..functions import window_attention as W
from . import window_attention as block_patch

PREVIOUS = "_devis_amd_glue_previous_forward"       # on a patched class: the forward the patch replaced
CLASSES = ("SwinTransformerBlock", "BasicLayer", "PatchMerging")


def _previous(self):
    return getattr(type(self), PREVIOUS)


def _affine_norm(norm, C):
    return isinstance(norm, nn.LayerNorm) and tuple(norm.normalized_shape) == (C,) and norm.weight is not None and \
        norm.bias is not None


def _out_dtype(x):
    """y's dtype: the autocast dtype beside a float32 stream (what the next Linear would cast to), x's otherwise."""
    if x.dtype == torch.float32 and torch.is_autocast_enabled(x.device.type):
        return torch.get_autocast_dtype(x.device.type)
    return None


def _fusable(self, x):
    """Whether this block takes the fused route: the attention's condition and the glue's own limits."""
    if not block_patch._fusable(self, x):
        return False
    C = x.shape[2]
    return C <= _prenorm.MAX_CHANNELS and _affine_norm(self.norm1, C) and _affine_norm(self.norm2, C)


def _keep(self, x):
    """The drop-path scale of each batch entry, drawn by the block's own module; None where the stock forward scales nothing."""
    if not self.training or isinstance(self.drop_path, nn.Identity):
        return None
    return self.drop_path(x.new_ones(x.shape[0], 1, 1)).view(x.shape[0])


def _scaled(delta, keep):
    return delta if keep is None else delta * keep.to(delta.dtype).view(-1, 1, 1)


def resolve(state):
    """The stream of a deferred state ``(x, delta, keep)``: ``x + keep * delta``, by torch."""
    x, delta, keep = state
    return x if delta is None else x + _scaled(delta, keep)


def block_state(self, x, delta=None, keep=None):
    """A fusable block on the deferred state ``(x, delta, keep)`` of the stream ``x + keep * delta``; returns the next state."""
    B, L, C = x.shape
    H, W_, ws = self.H, self.W, self.window_size
    assert L == H * W_, "input feature has wrong size"
    pad_b, pad_r = -H % ws, -W_ % ws
    out_dtype = _out_dtype(x)
    attn, norm1, norm2 = self.attn, self.norm1, self.norm2
    s, y = P.residual_layer_norm(x, delta, norm1.weight, norm1.bias, norm1.eps, keep=keep,
                                 map_size=(H, W_, H + pad_b, W_ + pad_r), out_dtype=out_dtype)
    a = W.window_attention(attn.qkv(y), attn.relative_position_bias_table, attn.num_heads, ws, self.shift_size, attn.scale)
    if pad_b or pad_r:
        a = a[:, :H, :W_, :]
    a = attn.proj_drop(attn.proj(a.reshape(B, H * W_, C)))
    s, y = P.residual_layer_norm(s, a, norm2.weight, norm2.bias, norm2.eps, keep=_keep(self, x), out_dtype=out_dtype)
    delta = self.mlp(y)
    return s, delta, _keep(self, x)


def block_forward(self, x, mask_matrix):
    """``SwinTransformerBlock.forward`` on the fused glue; ``mask_matrix`` is accepted and not read."""
    if not _fusable(self, x):
        return _previous(self)(self, x, mask_matrix)
    return resolve(block_state(self, x))


def layer_forward(self, x, H, W):
    """``BasicLayer.forward`` without the shift mask, the blocks chained on the deferred state."""
    if not all(_fusable(blk, x) for blk in self.blocks):
        return _previous(self)(self, x, H, W)
    state = (x, None, None)
    for blk in self.blocks:
        blk.H, blk.W = H, W
        if self.use_checkpoint:
            state = (checkpoint.checkpoint(blk, state[0], None, use_reentrant=False), None, None)
        else:
            state = block_state(blk, *state)
    x = resolve(state)
    if self.downsample is not None:
        x_down = self.downsample(x, H, W)
        return x, H, W, x_down, (H + 1) // 2, (W + 1) // 2
    return x, H, W, x, H, W


def merge_forward(self, x, H, W):
    """``PatchMerging.forward``: the gather and the norm as one pass, then the Linear."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or not _affine_norm(self.norm, 4 * x.shape[2]):
        return _previous(self)(self, x, H, W)
    assert x.shape[1] == H * W, "input feature has wrong size"
    norm = self.norm
    return self.reduction(P.patch_merge_norm(x, H, W, norm.weight, norm.bias, norm.eps, out_dtype=_out_dtype(x)))


FORWARDS = dict(zip(CLASSES, (block_forward, layer_forward, merge_forward)))


def patch(module):
    """Installs the three forwards on ``module``'s classes; returns what it replaced."""
    previous = {}
    for name, forward in FORWARDS.items():
        cls = getattr(module, name)
        current = cls.forward
        if current is forward:                               # (patched twice: the recorded forward stays)
            current = getattr(cls, PREVIOUS)
        setattr(cls, PREVIOUS, current)
        cls.forward = forward
        previous[name] = current
    return previous


def unpatch(module, previous):
    """Puts back what :func:`patch` returned.  Patches are undone in the reverse of the order they were applied in; where
    another patch's undoing has already replaced the glue's forward, that one is left in place."""
    for name, forward in FORWARDS.items():
        cls = getattr(module, name)
        if cls.forward is forward:
            cls.forward = previous[name]
        if PREVIOUS in cls.__dict__:
            delattr(cls, PREVIOUS)
