"""``ModulatedDeformableConv2d``: the convolution of DeVIS's mask head (reference ``src/models/deformable_segmentation.py``,
class of the same name) on :func:`devis_amd.ops.deform_conv2d` instead of ``torchvision.ops.deform_conv2d``.

Same constructor, same parameter names (``offset_conv``, ``modulator_conv``, ``regular_conv``) and the same initialisation
(offset and modulator convolutions zero: a fresh layer is a plain convolution), so reference checkpoints load with
``strict=True``.

``reproducible_grad_input`` (an attribute, not a parameter or buffer: it is in no state dict) chooses how the layer's
backward sums grad_input: None follows :class:`devis_amd.reproducible_grad_input`, True / False pins this layer to the
order-independent fixed-point sum / to float atomics.
"""
import torch
from torch import nn

from .. import ops


class ModulatedDeformableConv2d(nn.Module):
    reproducible_grad_input = None      # set on an instance to override the process-wide switch for that layer

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=False):
        super().__init__()
        self.stride = stride
        self.padding = padding
        taps = kernel_size * kernel_size
        self.offset_conv = nn.Conv2d(in_channels, 2 * taps, kernel_size=kernel_size, stride=stride, padding=padding, bias=True)
        nn.init.constant_(self.offset_conv.weight, 0.)
        nn.init.constant_(self.offset_conv.bias, 0.)
        self.modulator_conv = nn.Conv2d(in_channels, taps, kernel_size=kernel_size, stride=stride, padding=padding, bias=True)
        nn.init.constant_(self.modulator_conv.weight, 0.)
        nn.init.constant_(self.modulator_conv.bias, 0.)
        self.regular_conv = nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding,
                                      bias=bias)

    def forward(self, x):
        offset = self.offset_conv(x)
        modulator = self.modulator_conv(x)
        weight, bias = self.regular_conv.weight, self.regular_conv.bias
        if x.is_cuda and torch.is_autocast_enabled("cuda"):
            # autocast does not reach into a custom op: hand the operator its 16-bit input and weights here, and keep the
            # offsets and the modulation in float32 (a sampling position rounded to 8 bits moves by up to 1/32 pixel)
            dt = torch.get_autocast_dtype("cuda")
            x, weight, bias = x.to(dt), weight.to(dt), None if bias is None else bias.to(dt)
            offset, modulator = offset.float(), modulator.float()
        modulator = 2. * torch.sigmoid(modulator)
        # (the reference passes only `padding` on to the operator; its mask head never sets another stride than 1)
        return ops.deform_conv2d(x, offset, weight, bias, stride=self.stride, padding=self.padding, mask=modulator,
                                 reproducible_grad_input=self.reproducible_grad_input)
