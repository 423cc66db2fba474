"""The reference's ``SwinTransformerBlock`` (``src/models/swin_backbone.py``) on the fused window-attention operator (DESIGN.md
section 21): :func:`block_forward` has the block's signature and computes what its ``forward`` computes -- ``norm1``, view as a
map, ``F.pad`` only when the map is not a multiple of the window, ``self.attn.qkv`` on the map, one
:func:`devis_amd.window_attention` call, ``[:H, :W]``, ``self.attn.proj`` and ``proj_drop`` on the ``H * W`` tokens (``proj`` is
per token and commutes with the un-windowing), then the shortcut, ``drop_path`` and the MLP as before.  No roll, no window
partition or reverse and no ``[windows, heads, N, N]`` tensor exists.  :func:`devis_amd.patch_window_attention` installs it on
the reference's class; no module is replaced, so state dicts are untouched, and a block under ``use_checkpoint`` is called the
same way.

The ``mask_matrix`` argument is accepted and NOT read: the kernels derive the shift mask from ``(ys, xs)``, ``Hp``, ``Wp``, the
window and the shift by the rule of ``BasicLayer.forward`` (include/winattn.h), so a caller that passes another mask gets the
reference's.  ``relative_position_index`` is not read either: the table row is index arithmetic.

The replaced ``forward`` runs instead -- the block then computes exactly what it computed before the patch -- when the model is
compiling (``torch.compiler.is_compiling()``), the input is on the CPU or not ``[B, L, C]``, the dtype the ``qkv`` Linear returns
is not float32 / bfloat16 / float16 (float64), ``attn.attn_drop.p > 0`` in training mode (the kernels have no attention
dropout), or the window or the head dimension is one the kernels do not take (a window above 16; ``D`` not a multiple of 4 in
[4, 64]; a non-square window).  Under autocast ``qkv`` returns a 16-bit map and the float32 table is read as it is.
"""
import torch
import torch.nn.functional as F

from ..functions import window_attention as W

STOCK = "_devis_amd_stock_forward"      # on a patched class: the forward the patch replaced
CLASS = "SwinTransformerBlock"


def _on_gpu(x):
    return x.is_cuda


def _projected_dtype(linear, x):
    """The dtype ``linear(x)`` returns."""
    if torch.is_autocast_enabled(x.device.type):
        return torch.get_autocast_dtype(x.device.type)
    return linear.weight.dtype


def _fusable(self, x):
    """Whether this call takes the fused route (the module's docstring lists what sends it to the replaced forward)."""
    if torch.compiler.is_compiling() or not isinstance(x, torch.Tensor) or x.dim() != 3 or not _on_gpu(x):
        return False
    attn = self.attn
    if self.training and attn.attn_drop.p > 0:
        return False
    ws = self.window_size
    if not isinstance(ws, int) or tuple(attn.window_size) != (ws, ws) or not 0 <= self.shift_size < ws:
        return False
    if x.shape[2] != attn.dim or attn.dim % attn.num_heads:
        return False                                         # (the stock forward raises)
    table = attn.relative_position_bias_table
    dtype = _projected_dtype(attn.qkv, x)
    if table.dtype != dtype and table.dtype != torch.float32:
        return False
    return W.supported(dtype, attn.dim // attn.num_heads, ws)


def block_forward(self, x, mask_matrix):
    """``SwinTransformerBlock.forward`` on the fused operator; ``mask_matrix`` is accepted and not read."""
    if not _fusable(self, x):
        return getattr(type(self), STOCK)(self, x, mask_matrix)
    B, L, C = x.shape
    H, W_, ws = self.H, self.W, self.window_size
    assert L == H * W_, "input feature has wrong size"
    shortcut = x
    x = self.norm1(x).view(B, H, W_, C)
    pad_b, pad_r = -H % ws, -W_ % ws
    if pad_b or pad_r:
        x = F.pad(x, (0, 0, 0, pad_r, 0, pad_b))
    attn = self.attn
    x = W.window_attention(attn.qkv(x), attn.relative_position_bias_table, attn.num_heads, ws, self.shift_size, attn.scale)
    if pad_b or pad_r:
        x = x[:, :H, :W_, :]
    x = attn.proj_drop(attn.proj(x.reshape(B, H * W_, C)))
    x = shortcut + self.drop_path(x)
    return x + self.drop_path(self.mlp(self.norm2(x)))


def patch(module):
    """Installs :func:`block_forward` on ``module.SwinTransformerBlock``; returns what it replaced."""
    cls = getattr(module, CLASS)
    current = cls.forward
    if current is block_forward:                             # (patched twice: the stock forward is the recorded one)
        current = getattr(cls, STOCK)
    setattr(cls, STOCK, current)
    cls.forward = block_forward
    return {CLASS: current}


def unpatch(module, previous):
    """Puts back what :func:`patch` returned."""
    cls = getattr(module, CLASS)
    cls.forward = previous[CLASS]
    if STOCK in cls.__dict__:
        delattr(cls, STOCK)
