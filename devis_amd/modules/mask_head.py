"""``MaskHeadConv``: DeVIS's mask head (reference ``src/models/deformable_segmentation.py``, class of the same name) with the
glue between its convolutions -- GroupNorm, ReLU, nearest upsampling, the FPN add, the concatenation of the attention maps --
on :func:`devis_amd.ops.mask_head_stage`: one operator call per stage whose channels-last result the next convolution reads
without a layout copy.

Same constructor, same submodule names (``lay1..``, ``gn1..``, ``adapter1..``, ``out_lay``) and the same initialisation, so
state dicts load with ``strict=True`` in both directions.  ``use_deformable_conv=True`` builds
:class:`devis_amd.modules.ModulatedDeformableConv2d`, ``False`` the reference's plain ``Conv2d`` (kaiming ``a=1``, zero bias).

The FPN adapters run on the F un-expanded feature images and stay un-expanded: the operator reads image
``skip_index[n]`` for instance ``n``.  The index is what the caller's own ``expand_func`` makes of ``arange(F)``, so any repeat
pattern is reproduced without reading a device tensor; it is cached per (F, instances_per_batch, device).
"""
import torch
from torch import nn

from .. import ops
from .deform_conv import ModulatedDeformableConv2d


class Conv2d(nn.Conv2d):
    """The reference's plain convolution of the mask head: kaiming-uniform weights (a=1), zero bias."""

    def __init__(self, in_channels, out_channels, kernel_size, padding):
        super().__init__(in_channels, out_channels, kernel_size=kernel_size, padding=padding)
        nn.init.kaiming_uniform_(self.weight, a=1)
        nn.init.constant_(self.bias, 0)


def _instances_key(instances_per_batch):
    if isinstance(instances_per_batch, torch.Tensor):
        return tuple(instances_per_batch.tolist()) if instances_per_batch.device.type == "cpu" else id(instances_per_batch)
    if isinstance(instances_per_batch, (list, tuple)):
        return tuple(_instances_key(v) for v in instances_per_batch)
    return instances_per_batch


class MaskHeadConv(nn.Module):
    """Simple convolutional head with group norm; upsampling follows the FPN approach (the reference's docstring)."""

    def __init__(self, dim, fpn_dims, nheads, use_deformable_conv, multi_scale_att_maps, num_levels, out_layer=True):
        super().__init__()
        out_dims = [dim // (2 ** exp) for exp in range(num_levels + 2)]
        in_dims = [dim // (2 ** exp) for exp in range(num_levels + 2)]
        for i in range(len(multi_scale_att_maps)):
            in_dims[i] += nheads
        self.multi_scale_att_maps = len(multi_scale_att_maps) > 1
        conv_layer = ModulatedDeformableConv2d if use_deformable_conv else Conv2d

        self.lay1 = conv_layer(in_dims[0], in_dims[0], 3, padding=1)
        self.gn1 = nn.GroupNorm(8, in_dims[0])
        self.lay2 = conv_layer(in_dims[0], out_dims[1], 3, padding=1)
        self.gn2 = nn.GroupNorm(8, out_dims[1])
        for i in range(1, len(fpn_dims) + 1):
            setattr(self, "lay%d" % (i + 2), conv_layer(in_dims[i], out_dims[i + 1], 3, padding=1))
            setattr(self, "gn%d" % (i + 2), nn.GroupNorm(8, out_dims[i + 1]))
            setattr(self, "adapter%d" % i, Conv2d(fpn_dims[i - 1], out_dims[i], 1, padding=0))
        self.out_lay = None
        if out_layer:
            self.out_lay = conv_layer(out_dims[len(fpn_dims) + 1], 1, 3, padding=1)
        self._index_cache = {}

    def skip_index(self, num_images, instances_per_batch, expand_func, device):
        """[N] int64: which of the F un-expanded images each expanded image is -- ``expand_func`` applied to arange(F)."""
        key = None
        if not torch.compiler.is_compiling():
            key = (num_images, _instances_key(instances_per_batch), str(device), expand_func)
            hit = self._index_cache.get(key)
            if hit is not None:
                return hit
        index = expand_func(torch.arange(num_images, device=device).view(num_images, 1, 1, 1), instances_per_batch).flatten()
        if key is not None:
            if len(self._index_cache) >= 64:
                self._index_cache.clear()
            self._index_cache[key] = index
        return index

    def _stage(self, gn, x, skip=None, skip_index=None, extra=None):
        weight, bias, out_dtype = gn.weight, gn.bias, None
        if x.is_cuda and torch.is_autocast_enabled("cuda"):
            # autocast does not reach into a custom op: 16-bit x and skip, the parameters and the maps as they are
            # (float32), and the result in the autocast dtype -- what the next convolution would round it to anyway
            dt = torch.get_autocast_dtype("cuda")
            x, out_dtype = x.to(dt), dt
            skip = None if skip is None else skip.to(dt)
            if extra is not None and extra.dtype not in (dt, torch.float32):
                extra = extra.float()
        return ops.mask_head_stage(x, gn.num_groups, weight, bias, gn.eps, skip=skip, skip_index=skip_index, extra=extra,
                                   out_dtype=out_dtype)

    def forward(self, features, bbox_mask, instances_per_batch, expand_func):
        """``features``: the /32 .. /4 feature maps [F, C_l, H_l, W_l]; ``bbox_mask``: the attention maps per level
        [N, nheads, H_l, W_l]; ``expand_func(tensor, instances_per_batch)`` repeats the F images to the N instances."""
        expanded_feats = expand_func(features[0], instances_per_batch)
        x = torch.cat([expanded_feats, bbox_mask[0]], 1)
        x = self._stage(self.gn1, self.lay1(x))
        x = self.lay2(x)
        if len(features) == 1:
            x = self._stage(self.gn2, x)
        gn = self.gn2
        for lvl, feature in enumerate(features[1:]):
            cur_fpn = getattr(self, "adapter%d" % (lvl + 1))(feature)
            index = self.skip_index(feature.shape[0], instances_per_batch, expand_func, feature.device)
            extra = bbox_mask[lvl + 1] if self.multi_scale_att_maps and lvl + 1 < len(bbox_mask) else None
            x = self._stage(gn, x, cur_fpn, index, extra)
            x = getattr(self, "lay%d" % (lvl + 3))(x)
            gn = getattr(self, "gn%d" % (lvl + 3))
            if lvl + 2 == len(features):
                x = self._stage(gn, x)
        if self.out_lay is not None:
            x = self.out_lay(x)
        return x
