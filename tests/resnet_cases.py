"""Stand-ins for the modules devis_amd.patch_resnet_glue finds by structure (tests only; torchvision is not a dependency):
a ``FrozenBatchNorm2d`` with the reference's buffer names, a Bottleneck and a BasicBlock with torchvision's attribute names and
call order, a ResNet-shaped holder of a stem and one stage, and an ``IntermediateLayerGetter``-shaped holder that calls the
same child instances in turn."""
import torch
from torch import nn


class FrozenBatchNorm2d(nn.Module):
    """Fixed statistics and affine parameters, all four as buffers.  ``eps`` is stored when given (torchvision's class),
    else 1e-5 is used (the reference's)."""

    def __init__(self, channels, eps=None):
        super().__init__()
        self.register_buffer("weight", torch.ones(channels))
        self.register_buffer("bias", torch.zeros(channels))
        self.register_buffer("running_mean", torch.zeros(channels))
        self.register_buffer("running_var", torch.ones(channels))
        if eps is not None:
            self.eps = eps

    def forward(self, x):
        per_channel = (1, -1, 1, 1)
        scale = self.weight.view(per_channel) * torch.rsqrt(self.running_var.view(per_channel) + getattr(self, "eps", 1e-5))
        shift = self.bias.view(per_channel) - self.running_mean.view(per_channel) * scale
        return x * scale + shift


def _downsample(inplanes, outplanes, stride, norm):
    if stride == 1 and inplanes == outplanes:
        return None
    return nn.Sequential(nn.Conv2d(inplanes, outplanes, 1, stride=stride, bias=False), norm(outplanes))


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, norm=FrozenBatchNorm2d):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = norm(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = norm(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = norm(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = _downsample(inplanes, planes * self.expansion, stride, norm)

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, norm=FrozenBatchNorm2d):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = norm(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = norm(planes)
        self.downsample = _downsample(inplanes, planes, stride, norm)

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


class ResNet(nn.Module):
    """A stem and one stage of two blocks, the first with a ``downsample`` branch."""

    def __init__(self, block=Bottleneck, width=8, planes=4, norm=FrozenBatchNorm2d):
        super().__init__()
        self.conv1 = nn.Conv2d(3, width, 7, stride=2, padding=3, bias=False)
        self.bn1 = norm(width)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = nn.Sequential(block(width, planes, 1 if block is Bottleneck else 2, norm),
                                    block(planes * block.expansion, planes, 1, norm))

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        return self.layer1(x)


class LayerGetter(nn.ModuleDict):
    """Holds the children of a model -- the same instances -- and calls them in turn, returning those asked for."""

    def __init__(self, model, return_layers):
        super().__init__(dict(model.named_children()))
        self.return_layers = dict(return_layers)

    def forward(self, x):
        out = {}
        for name, module in self.items():
            x = module(x)
            if name in self.return_layers:
                out[self.return_layers[name]] = x
        return out


def randomise(model, seed=0):
    """Random weights and frozen statistics: norm weights of both signs, variances in [0.5, 2]."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in list(model.named_parameters()) + list(model.named_buffers()):
            r = torch.randn(t.shape, generator=g, dtype=torch.float64)
            if name.endswith("running_var"):
                r = 0.5 + 1.5 * torch.rand(t.shape, generator=g, dtype=torch.float64)
            elif t.dim() == 4:
                r = r * (1.5 / (t[0].numel() ** 0.5))
            t.copy_(r.to(t.dtype))
    return model
