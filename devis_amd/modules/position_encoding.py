"""DeVIS's sine position encodings (reference ``src/models/position_encoding.py``: ``PositionEmbeddingSine`` and
``PositionEmbeddingSineWithLearnableTemporal``, the default ``TEMPORAL_EMBEDDING = 'learned'``) on the HIP kernels of
include/posembed.h, with the reference's constructor arguments and state-dict key (``temporal_embed``).

``forward(tensor_list)`` returns the reference's tensor ``[N, C, H, W]``: :func:`devis_amd.sine_position_embedding` of the
mask, and for the temporal class ``+ temporal_embed[:, :, None, None]`` added by torch exactly as the reference adds it, so
autograd reaches the parameter the usual way.

In deferred mode (``module.deferred = True``, or the reference's classes under ``devis_amd.patch_position_encoding``) the
forward launches nothing and returns a :class:`DeferredPositionEmbedding`: the encoder's ``prepare_data`` then makes ONE
:func:`devis_amd.encoder_position_embedding` call for all levels, and the ``[N, C, H, W]`` tensors never exist.
"""
import math

import torch
from torch import nn
from torch.nn.init import normal_


def sine_of(module, mask):
    """``PositionEmbeddingSine.forward`` of ``mask`` with ``module``'s settings (ours or the reference's class): float32
    ``[N, 2 * num_pos_feats, H, W]``."""
    from .. import ops
    return ops.sine_position_embedding(mask, num_pos_feats=module.num_pos_feats, temperature=module.temperature,
                                       normalize=module.normalize, scale=module.scale if module.normalize else None)


def materialized(module, mask, dtype=None):
    """The tensor the reference's forward returns for ``mask``, then ``.to(dtype)`` where one is given."""
    pos = sine_of(module, mask)
    temporal_embed = getattr(module, "temporal_embed", None)
    if temporal_embed is not None:
        pos = pos + temporal_embed[:, :, None, None]
    return pos if dtype is None else pos.to(dtype)


class DeferredPositionEmbedding:
    """A position embedding that is not computed yet: the padding ``mask`` [N, H, W], the ``module`` whose forward was asked
    for it, and ``dtype``, what a ``.to(dtype)`` of the caller asked for (None: none).  ``shape`` is the tensor's,
    ``materialize()`` the tensor itself (computed once), and every other attribute is the materialised tensor's: a consumer
    that knows nothing of this class -- the stock ``prepare_data`` calling ``.flatten(2)`` -- gets the right values.  The fused
    ``prepare_data`` of ``devis_amd.patch_position_encoding`` reads ``mask``, ``module`` and ``dtype`` instead."""

    def __init__(self, module, mask, dtype=None):
        self.module, self.mask, self.dtype = module, mask, dtype
        self._tensor = None

    @property
    def shape(self):
        return torch.Size((self.mask.shape[0], 2 * self.module.num_pos_feats) + tuple(self.mask.shape[1:]))

    def to(self, *args, **kwargs):
        if len(args) == 1 and not kwargs and isinstance(args[0], torch.dtype):
            return DeferredPositionEmbedding(self.module, self.mask, args[0])
        return self.materialize().to(*args, **kwargs)

    def materialize(self):
        if self._tensor is None:
            self._tensor = materialized(self.module, self.mask, self.dtype)
        return self._tensor

    def __getattr__(self, name):
        if name.startswith("__") or name in ("module", "mask", "dtype", "_tensor"):
            raise AttributeError(name)
        return getattr(self.materialize(), name)


def deferred_forward(self, tensor_list):
    """What ``devis_amd.patch_position_encoding`` makes the forward of the reference's two classes: nothing is launched."""
    assert tensor_list.mask is not None
    return DeferredPositionEmbedding(self, tensor_list.mask)


class PositionEmbeddingSine(nn.Module):
    """Standard 2D sine positional encoding (reference position_encoding.py:62-103) on the HIP kernels."""

    deferred = False

    def __init__(self, num_pos_feats=64, temperature=10000, normalize=False, scale=None):
        super().__init__()
        if scale is not None and normalize is False:
            raise ValueError("normalize should be True if scale is passed")         # (the reference's rule and message)
        self.num_pos_feats, self.temperature, self.normalize = num_pos_feats, temperature, normalize
        self.scale = 2 * math.pi if scale is None else scale

    def forward(self, tensor_list):
        assert tensor_list.mask is not None
        if self.deferred:
            return DeferredPositionEmbedding(self, tensor_list.mask)
        return materialized(self, tensor_list.mask)


class PositionEmbeddingSineWithLearnableTemporal(PositionEmbeddingSine):
    """The 2D sine encoding plus a learned embedding per frame (reference position_encoding.py:106-124)."""

    def __init__(self, hidden_dim=256, num_frames=6, temperature=10000, normalize=False, scale=None):
        super().__init__(num_pos_feats=hidden_dim // 2, temperature=temperature, normalize=normalize, scale=scale)
        self.num_frames = num_frames
        self.temporal_embed = nn.Parameter(torch.Tensor(num_frames, hidden_dim))
        self._reset_parameters()

    def _reset_parameters(self):
        normal_(self.temporal_embed)
