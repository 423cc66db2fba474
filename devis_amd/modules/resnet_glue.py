"""The ResNet backbone's blocks on the fused frozen-norm kernels: :func:`patch` finds, BY STRUCTURE,
torchvision's ``Bottleneck`` / ``BasicBlock`` and the stem (``conv1, bn1, relu, maxpool``) under a module -- a torchvision
``ResNet``, the reference's ``Backbone`` or ``Joiner`` (``src/models/backbone.py``) or the ``IntermediateLayerGetter`` inside --
and gives each matched INSTANCE a subclass of its own class whose ``forward`` issues one
:func:`devis_amd.frozen_batch_norm` call per convolution.  torchvision is not imported.  No module is replaced and nothing is
registered: state dicts, ``named_parameters`` and both callers of the stem (``ResNet._forward_impl`` and
``IntermediateLayerGetter.forward``, which call the same instances in turn) are untouched, and :func:`unpatch` puts the classes
back.

What matches.  A frozen norm is a module whose class (or a base) is named ``FrozenBatchNorm2d``, with the four buffers
``weight, bias, running_mean, running_var`` and no parameters; its eps is ``getattr(bn, "eps", 1e-5)`` (the reference hard-codes
1e-5, torchvision's class stores it).  A Bottleneck has ``conv1, bn1, conv2, bn2, conv3, bn3, relu, downsample``, a BasicBlock
the same without ``conv3`` and ``bn3``; a block matches only if every norm is frozen, ``relu`` is an ``nn.ReLU`` and
``downsample`` is None or a module.  The stem matches when ``bn1`` is frozen, ``relu`` is an ``nn.ReLU``, ``maxpool`` is an
``nn.MaxPool2d`` of kernel 3, stride 2, padding 1, dilation 1 and floor mode, and ``relu`` and ``maxpool`` have no other
parent than holders of this same stem.

What runs.  A block: ``bn1`` and ``bn2`` with their ReLU, and the tail ``relu(bn3(.) + identity)`` as one call; when
``downsample`` is ``Sequential(conv, frozen norm)`` only its convolution runs and the norm folds into the tail as
``residual_norm``.  The stem: ``bn1`` returns the POOLED map (:func:`devis_amd.frozen_batch_norm_relu_pool`) and ``relu`` and
``maxpool`` pass it through.  A call is eligible when it is not compiling (``torch.compiler.is_compiling()``), its input is a
4-D GPU tensor with elements, in float32 / bfloat16 / float16, and every buffer of the block is float32; a call that is not
runs the forward the block had -- for the stem, ``bn1`` runs the three stock steps itself.  ``nn.BatchNorm2d``, training-mode
statistics and folding the norms into the convolutions are out of scope.

``keep_input_dtype=True`` writes every fused output in the dtype of the convolution output it reads -- 16-bit throughout
under autocast -- where the stock modules (and the default) return torch's promotion with the float32 buffers: float32.
"""
import torch
import torch.nn.functional as F
from torch import nn

from ..functions import frozen_norm

BUFFERS = ("weight", "bias", "running_mean", "running_var")
KEEP = "_resnet_glue_keep_input_dtype"


def is_frozen_norm(module):
    if not isinstance(module, nn.Module) or not any(k.__name__ == "FrozenBatchNorm2d" for k in type(module).__mro__):
        return False
    return all(isinstance(module._buffers.get(name), torch.Tensor) for name in BUFFERS) and not module._parameters


def norm_of(bn):
    """``(weight, bias, running_mean, running_var, eps)`` of a frozen norm."""
    return (bn.weight, bn.bias, bn.running_mean, bn.running_var, getattr(bn, "eps", 1e-5))


def _has(module, *names):
    # (an absent ``downsample`` is a plain None attribute, not a registered child)
    return all(name in module._modules or name in module.__dict__ for name in names)


def _is_block(module, names):
    if not _has(module, "relu", "downsample", *names) or not isinstance(module.relu, nn.ReLU):
        return False
    return all(is_frozen_norm(getattr(module, n)) for n in names if n.startswith("bn"))


def is_bottleneck(module):
    return _is_block(module, ("conv1", "bn1", "conv2", "bn2", "conv3", "bn3"))


def is_basic_block(module):
    return not _has(module, "conv3") and not _has(module, "bn3") and _is_block(module, ("conv1", "bn1", "conv2", "bn2"))


def _is_stem_pool(pool):
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)      # noqa: E731
    return (isinstance(pool, nn.MaxPool2d) and pair(pool.kernel_size) == (3, 3) and pair(pool.stride) == (2, 2) and
            pair(pool.padding) == (1, 1) and pair(pool.dilation) == (1, 1) and not pool.ceil_mode and not pool.return_indices)


def is_stem_holder(module):
    if not _has(module, "conv1", "bn1", "relu", "maxpool") or _has(module, "conv2"):
        return False
    return is_frozen_norm(module.bn1) and isinstance(module.relu, nn.ReLU) and _is_stem_pool(module.maxpool)


def _folded(downsample):
    """(conv, norm) of a ``Sequential(conv, frozen norm)``, or None."""
    if isinstance(downsample, nn.Sequential) and len(downsample) == 2 and is_frozen_norm(downsample[1]):
        return downsample[0], downsample[1]
    return None


def _norms(block):
    norms = [norm_of(getattr(block, n)) for n in ("bn1", "bn2", "bn3") if n in block._modules]
    pair = _folded(block.downsample)
    return norms + ([norm_of(pair[1])] if pair else [])


def _out_dtype(module, t):
    return t.dtype if getattr(module, KEEP, False) else None


def _tail(block, bn, out, x):
    pair = _folded(block.downsample)
    if pair is not None:
        identity, residual_norm = pair[0](x), norm_of(pair[1])
    else:
        identity, residual_norm = (x if block.downsample is None else block.downsample(x)), None
    return frozen_norm.frozen_batch_norm(out, *norm_of(bn), residual=identity, residual_norm=residual_norm, relu=True,
                                         out_dtype=_out_dtype(block, out))


def _act(block, bn, out):
    return frozen_norm.frozen_batch_norm(out, *norm_of(bn), relu=True, out_dtype=_out_dtype(block, out))


def _bottleneck_forward(self, x):
    if not frozen_norm.eligible(x, *_norms(self)):
        return self._resnet_glue_stock.forward(self, x)
    out = _act(self, self.bn1, self.conv1(x))
    out = _act(self, self.bn2, self.conv2(out))
    return _tail(self, self.bn3, self.conv3(out), x)


def _basic_forward(self, x):
    if not frozen_norm.eligible(x, *_norms(self)):
        return self._resnet_glue_stock.forward(self, x)
    out = _act(self, self.bn1, self.conv1(x))
    return _tail(self, self.bn2, self.conv2(out), x)


def _stem_norm_forward(self, x):
    """The stem's ``bn1``: the pooled map, fused when eligible, else the three stock steps."""
    if not frozen_norm.eligible(x, norm_of(self)) or (torch.is_grad_enabled() and x.requires_grad):
        return F.max_pool2d(F.relu(self._resnet_glue_stock.forward(self, x)), kernel_size=3, stride=2, padding=1)
    return frozen_norm.frozen_batch_norm_relu_pool(x, *norm_of(self), out_dtype=_out_dtype(self, x))


def _pass_through(self, x):
    """The stem's ``relu`` and ``maxpool`` behind a patched ``bn1``, which has applied both."""
    return x


_classes = {}       # (original class, kind) -> its fused subclass


def _fused_class(cls, kind, forward):
    key = (cls, kind)
    if key not in _classes:
        _classes[key] = type("Fused" + cls.__name__, (cls,), {"forward": forward, "_resnet_glue_stock": cls,
                                                              "_resnet_glue_kind": kind, "__module__": __name__})
    return _classes[key]


def _is_patched(module):
    return hasattr(type(module), "_resnet_glue_kind")


def patch(root_module, keep_input_dtype=False):
    """Patches every matching block and stem under ``root_module`` (the module docstring says what matches); returns what
    :func:`unpatch` needs."""
    previous = []

    def turn(module, kind, forward):
        if _is_patched(module):
            return
        previous.append((module, type(module)))
        module.__class__ = _fused_class(type(module), kind, forward)
        module.__dict__[KEEP] = bool(keep_input_dtype)

    modules = list(root_module.modules())
    for module in modules:
        if _is_patched(module):
            continue
        if is_bottleneck(module):
            turn(module, "bottleneck", _bottleneck_forward)
        elif is_basic_block(module):
            turn(module, "basic", _basic_forward)
    # the stem: every holder of one (bn1, relu, maxpool) triple; relu and maxpool may have no other parent
    holders = [m for m in modules if not _is_patched(m) and is_stem_holder(m) and not _is_patched(m.bn1)]
    for holder in holders:
        same = [h for h in holders if h.bn1 is holder.bn1 and h.relu is holder.relu and h.maxpool is holder.maxpool]
        shared = {id(holder.relu), id(holder.maxpool)}
        others = [m for m in modules if all(m is not h for h in same) and any(id(child) in shared for child in m._modules.values())]
        if others or holder.relu is holder.maxpool:
            continue
        turn(holder.bn1, "stem_norm", _stem_norm_forward)
        turn(holder.relu, "stem_relu", _pass_through)
        turn(holder.maxpool, "stem_pool", _pass_through)
    return previous


def unpatch(root_module, previous):
    """Puts back what :func:`patch` returned."""
    for module, cls in reversed(previous):
        module.__class__ = cls
        module.__dict__.pop(KEEP, None)
