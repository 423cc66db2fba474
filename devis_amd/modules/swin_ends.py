"""The two ends of the reference's Swin backbone (``src/models/swin_backbone.py``) on the fused kernels of DESIGN.md section 24.
:func:`devis_amd.patch_swin_ends` installs two forwards on the reference's classes, by name; no module is replaced, so state
dicts are untouched.

``PatchEmbed.forward(x)`` -- :func:`embed_forward`::

    tokens = patch_embed_norm(x, proj.weight, proj.bias, norm.weight, norm.bias, norm.eps)      # [B, Wh * Ww, C], one pass
    return tokens.transpose(1, 2).view(B, C, Wh, Ww)

The result has the reference's shape and is a VIEW of the dense token tensor, so the ``flatten(2).transpose(1, 2)`` that follows
in ``SwinTransformer.forward`` gives the dense tokens back without a copy.  Without a norm (``patch_norm=False``) the tokens are
the projection.  Under autocast the kernel computes in float32 from the float32 image and parameters and returns float32 tokens,
as the stock norm does; the stock convolution rounds to the autocast dtype first and the kernel does not.

``SwinTransformer.forward(x)`` -- :func:`backbone_forward`: the reference's loop with
``layer_norm_to_map(x_out, H, W, norm_i.weight, norm_i.bias, norm_i.eps)`` in place of ``norm_i``, ``view``, ``permute`` and
``contiguous``; the same dict, keys, shapes and dtypes.  With ``ape=True`` the reference's expression stays as it is.

The forward that was installed before the patch runs instead while compiling, on CPU tensors, in float64, when a norm is not an
affine ``nn.LayerNorm`` over the channels, when the projection is not a ``Conv2d`` with ``kernel_size == stride`` (square), no
padding, no dilation and one group, and above the operators' limits.
"""
import torch
import torch.nn.functional as F
from torch import nn

from .. import _swinends
from ..functions import swin_ends as E
from .swin_glue import _affine_norm

PREVIOUS = "_devis_amd_ends_previous_forward"       # on a patched class: the forward the patch replaced
CLASSES = ("PatchEmbed", "SwinTransformer")


def _previous(self):
    return getattr(type(self), PREVIOUS)


def _on_gpu(x):
    return x.is_cuda


def _takes(x, dims):
    return not torch.compiler.is_compiling() and isinstance(x, torch.Tensor) and x.dim() == dims and _on_gpu(x) and \
        x.dtype in E.DTYPES


def _plain_projection(proj):
    """A ``Conv2d`` that is a per-patch Linear: square kernel == stride, no padding, no dilation, one group."""
    if not isinstance(proj, nn.Conv2d) or isinstance(proj.padding, str):
        return False
    k = tuple(proj.kernel_size)
    return k[0] == k[1] and tuple(proj.stride) == k and tuple(proj.padding) == (0, 0) and tuple(proj.dilation) == (1, 1) and \
        proj.groups == 1


def _embed_fusable(self, x):
    if not _takes(x, 4) or not _plain_projection(self.proj):
        return False
    proj, norm = self.proj, self.norm
    C, Cin, p = proj.weight.shape[:3]
    if x.shape[1] != Cin or C > _swinends.MAX_EMBED or Cin * p * p > _swinends.MAX_PATCH:
        return False
    if norm is not None and not (_affine_norm(norm, C) and norm.weight.dtype == proj.weight.dtype):
        return False
    return E.embed_supported(x.dtype, proj.weight.dtype, x.dtype)


def embed_forward(self, x):
    """``PatchEmbed.forward``: one pass from the image to the normalised tokens, returned as the reference's NCHW view."""
    if not _embed_fusable(self, x):
        return _previous(self)(self, x)
    proj, norm = self.proj, self.norm
    p = proj.kernel_size[0]
    B, _, H, W = x.shape
    if norm is None:
        tokens = E.patch_embed_norm(x, proj.weight, proj.bias, None, None)
    else:
        tokens = E.patch_embed_norm(x, proj.weight, proj.bias, norm.weight, norm.bias, norm.eps)
    return tokens.transpose(1, 2).view(B, proj.weight.shape[0], -(-H // p), -(-W // p))


def _backbone_fusable(self, x):
    if not _takes(x, 4):
        return False
    for i in self.out_indices:
        C = self.num_features[i]
        if C > _swinends.MAX_CHANNELS or not _affine_norm(getattr(self, "norm%d" % i), C):
            return False
    return True


def backbone_forward(self, x):
    """``SwinTransformer.forward`` with each output norm written once, as the NCHW map."""
    if not _backbone_fusable(self, x):
        return _previous(self)(self, x)
    x = self.patch_embed(x)
    Wh, Ww = x.size(2), x.size(3)
    if self.ape:
        absolute_pos_embed = F.interpolate(self.absolute_pos_embed, size=(Wh, Ww), mode="bicubic")
        x = (x + absolute_pos_embed).flatten(2).transpose(1, 2)
    else:
        x = x.flatten(2).transpose(1, 2)
    x = self.pos_drop(x)
    outs = []
    for i in range(self.num_layers):
        x_out, H, W, x, Wh, Ww = self.layers[i](x, Wh, Ww)
        if i in self.out_indices:
            norm = getattr(self, "norm%d" % i)
            outs.append(E.layer_norm_to_map(x_out, H, W, norm.weight, norm.bias, norm.eps))
    return {str(u): v for u, v in enumerate(outs)}


FORWARDS = dict(zip(CLASSES, (embed_forward, backbone_forward)))


def patch(module):
    """Installs the two forwards on ``module``'s classes; returns what it replaced."""
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
    """Puts back what :func:`patch` returned."""
    for name, forward in FORWARDS.items():
        cls = getattr(module, name)
        if cls.forward is forward:
            cls.forward = previous[name]
        if PREVIOUS in cls.__dict__:
            delattr(cls, PREVIOUS)
