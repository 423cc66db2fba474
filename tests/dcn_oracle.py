"""Oracle of the modulated deformable convolution (test infrastructure only): the formula of include/mdcn.h in plain
PyTorch -- float64 on the CPU in the tests -- one gather per bilinear corner with validity masks, gradients by autograd.
Written from the formula:

    out[n, o, ho, wo] = bias[o] + sum_{c, i, j} weight[o, c, i, j] * mask[n, g*K + k, ho, wo] * S(input[n, c], y, x)
    k = i*Kw + j,  g = c // (C/G),
    y = ho*sh - ph + i*dh + offset[n, 2*(g*K + k), ho, wo],   x = wo*sw - pw + j*dw + offset[n, 2*(g*K + k) + 1, ho, wo]

with S the bilinear interpolation of the image extended by zeros in every direction: the four corners (floor(y) + a,
floor(x) + b), a, b in {0, 1}, weighted by (ly if a else 1 - ly) * (lx if b else 1 - lx) with ly = y - floor(y), lx = x - floor(x),
a corner outside [0, H-1] x [0, W-1] counting as zero.  S has kinks at integer coordinates; there autograd gives the derivative
of the cell [floor, floor + 1) the point is assigned to.
"""
import torch
from torch import nn


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def sample_columns(input, offset, kernel_size, stride=(1, 1), padding=(0, 0), dilation=(1, 1), mask=None):
    """The masked samples [N, C, K, Ho, Wo] every output pixel's taps read."""
    (Kh, Kw), (sh, sw), (ph, pw), (dh, dw) = _pair(kernel_size), _pair(stride), _pair(padding), _pair(dilation)
    N, C, H, W = input.shape
    K = Kh * Kw
    Ho = (H + 2 * ph - dh * (Kh - 1) - 1) // sh + 1
    Wo = (W + 2 * pw - dw * (Kw - 1) - 1) // sw + 1
    G = offset.shape[1] // (2 * K)
    assert offset.shape == (N, 2 * G * K, Ho, Wo) and C % G == 0
    dt, dev = input.dtype, input.device
    off = offset.to(dt).view(N, G, K, 2, Ho, Wo)
    i = torch.arange(Kh, device=dev).repeat_interleave(Kw).to(dt).view(1, 1, K, 1, 1)
    j = torch.arange(Kw, device=dev).repeat(Kh).to(dt).view(1, 1, K, 1, 1)
    ho = torch.arange(Ho, device=dev).to(dt).view(1, 1, 1, Ho, 1)
    wo = torch.arange(Wo, device=dev).to(dt).view(1, 1, 1, 1, Wo)
    y = ho * sh - ph + i * dh + off[:, :, :, 0]         # [N, G, K, Ho, Wo]
    x = wo * sw - pw + j * dw + off[:, :, :, 1]
    # the range test as include/mdcn.h states it: false for a NaN coordinate, whose tap then contributes nothing and has zero
    # gradients (NaN * 0 below would be NaN; +-inf - floor(+-inf) too)
    inside = (y > -1) & (y < H) & (x > -1) & (x < W)
    y, x = torch.where(inside, y, torch.zeros_like(y)), torch.where(inside, x, torch.zeros_like(x))
    y0, x0 = torch.floor(y).detach(), torch.floor(x).detach()
    flat = input.reshape(N, G, C // G, H * W)
    total = torch.zeros((N, G, C // G, K, Ho, Wo), dtype=dt, device=dev)
    for a in (0, 1):
        for b in (0, 1):
            yc, xc = y0 + a, x0 + b
            wgt = ((y - y0) if a else (1 - (y - y0))) * ((x - x0) if b else (1 - (x - x0)))
            valid = inside & (yc >= 0) & (yc <= H - 1) & (xc >= 0) & (xc <= W - 1)
            idx = (yc.clamp(0, H - 1) * W + xc.clamp(0, W - 1)).long().view(N, G, 1, K * Ho * Wo)
            got = torch.gather(flat, 3, idx.expand(N, G, C // G, K * Ho * Wo)).view(N, G, C // G, K, Ho, Wo)
            total = total + got * (wgt * valid.to(dt)).unsqueeze(2)
    if mask is not None:
        total = total * mask.to(dt).view(N, G, 1, K, Ho, Wo)
    return total.view(N, C, K, Ho, Wo)


def deform_conv2d(input, offset, weight, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), mask=None):
    Co, C, Kh, Kw = weight.shape
    cols = sample_columns(input, offset, (Kh, Kw), stride, padding, dilation, mask)
    out = torch.einsum("nckhw,ock->nohw", cols, weight.reshape(Co, C, Kh * Kw))
    if bias is not None:
        out = out + bias.view(1, Co, 1, 1)
    return out


class ModulatedDeformableConv2d(nn.Module):
    """The mask-head layer built on the oracle: offset conv, 2*sigmoid(modulator conv), deform_conv2d."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=False):
        super().__init__()
        self.stride, self.padding = stride, padding
        taps = kernel_size * kernel_size
        self.offset_conv = nn.Conv2d(in_channels, 2 * taps, kernel_size, stride=stride, padding=padding, bias=True)
        self.modulator_conv = nn.Conv2d(in_channels, taps, kernel_size, stride=stride, padding=padding, bias=True)
        self.regular_conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=bias)

    def forward(self, x):
        offset = self.offset_conv(x)
        modulator = 2. * torch.sigmoid(self.modulator_conv(x))
        return deform_conv2d(x, offset, self.regular_conv.weight, self.regular_conv.bias, stride=self.stride,
                             padding=self.padding, mask=modulator)
