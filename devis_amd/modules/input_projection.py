"""The reference's input projections (``DeformableDETR.input_proj``, a ``ModuleList`` of ``Sequential(Conv2d, GroupNorm)``:
src/models/deformable_detr.py) on the HIP kernels of include/inputproj.h, under ``devis_amd.patch_input_proj``.

The patch gives every ``GroupNorm`` of the list the class :class:`DeferringGroupNorm` (its ``__class__`` is set: no module is
replaced, state dicts are untouched).  Its forward launches nothing and returns a :class:`DeferredInputProjection`; the
encoder's ``prepare_data`` then makes ONE :func:`devis_amd.group_norm_tokens` call for all levels
(:func:`fused_tokens`), which writes ``src_flatten`` directly, and the normalised ``[N, C, H, W]`` maps never exist.

A level whose output the reference feeds into the next projection's convolution -- a 3 x 3 / stride-2 projection that is
followed by another one, which happens with five or more levels only (deformable_detr.py:162-166) -- is not deferred: it runs the
one-level kernel at once and returns a tensor, the channels-last ``[N, C, H, W]`` view of its tokens.

The stock forward runs while ``torch.compiler.is_compiling()``, for an input that is not ``[N, C, H, W]`` and for a norm
without affine parameters.
"""
import torch
from torch import nn

from ..functions.input_projection import group_norm_tokens


def _as_map(tokens, size):
    """``tokens [N, H * W, C]`` as the ``[N, C, H, W]`` map it holds: a channels-last-strided view, no copy."""
    return tokens.transpose(1, 2).unflatten(2, tuple(size))


def result_dtype(x):
    """The dtype stock ``GroupNorm`` returns for ``x``: float32 under autocast (it is one of autocast's float32 ops), else
    ``x``'s."""
    return torch.float32 if x.is_floating_point() and torch.is_autocast_enabled(x.device.type) else x.dtype


def one_level(module, x, dtype):
    """``module(x)`` -- a ``GroupNorm`` -- in ``dtype`` by the one-level operator call, viewed as ``[N, C, H, W]``."""
    tokens = group_norm_tokens([x], module.num_groups, [module.weight], [module.bias], module.eps,
                               None if dtype == x.dtype else dtype)
    return _as_map(tokens, x.shape[2:])


class DeferredInputProjection:
    """A projected level whose GroupNorm is not computed yet: ``x``, the convolution's output ``[N, C, H, W]``, the ``module``
    (the ``GroupNorm``) whose forward was asked for it, and ``dtype``, the one stock would return.  ``shape``, ``dtype`` and
    ``device`` are answered without computing; ``materialize()`` is the tensor itself (computed once: the one-level operator
    call viewed as ``[N, C, H, W]``), and every other attribute is the materialised tensor's: a consumer that knows nothing of
    this class -- the stock ``prepare_data`` calling ``.flatten(2)`` -- gets the right values.  The fused ``prepare_data``
    reads ``x`` and ``module`` instead and binds the object to its view of ``src_flatten`` (:func:`fused_tokens`), which later
    consumers of ``srcs`` then get, values and gradients included."""

    _OWN = ("module", "x", "dtype", "_tensor")

    def __init__(self, module, x, dtype):
        self.module, self.x, self.dtype = module, x, dtype
        self._tensor = None

    @property
    def shape(self):
        return self.x.shape

    @property
    def device(self):
        return self.x.device

    def bind(self, tensor):
        self._tensor = tensor

    def materialize(self):
        if self._tensor is None:
            self._tensor = one_level(self.module, self.x, self.dtype)
        return self._tensor

    def __getattr__(self, name):
        if name.startswith("__") or name in self._OWN:
            raise AttributeError(name)
        return getattr(self.materialize(), name)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        """A torch function called on a deferred projection -- a convolution of the mask head, a ``cat`` -- gets the tensor."""
        def tensors(v):
            if isinstance(v, DeferredInputProjection):
                return v.materialize()
            if isinstance(v, (list, tuple)):
                return type(v)(tensors(e) for e in v)
            return v
        return func(*tensors(args), **{k: tensors(v) for k, v in (kwargs or {}).items()})


def _delegate(name):
    def method(self, *args, **kwargs):
        return getattr(self.materialize(), name)(*args, **kwargs)
    method.__name__ = name
    return method


# (Python looks operators up on the class, past __getattr__)
for _name in ("add", "radd", "sub", "rsub", "mul", "rmul", "truediv", "rtruediv", "matmul", "rmatmul", "neg", "getitem", "len"):
    setattr(DeferredInputProjection, "__%s__" % _name, _delegate("__%s__" % _name))


class DeferringGroupNorm(nn.GroupNorm):
    """What ``devis_amd.patch_input_proj`` makes of the ``GroupNorm`` of a projection: ``defer_output`` says whether the forward
    returns a :class:`DeferredInputProjection` or, for a level the next projection reads, the tensor of :func:`one_level`."""

    defer_output = True

    def forward(self, x):
        if torch.compiler.is_compiling() or not isinstance(x, torch.Tensor) or x.dim() != 4 or not self.affine:
            return super().forward(x)
        dtype = result_dtype(x)
        if not self.defer_output:
            return one_level(self, x, dtype)
        return DeferredInputProjection(self, x, dtype)


def materialized(src):
    return src.materialize() if isinstance(src, DeferredInputProjection) else src


def fused_tokens(srcs):
    """``src_flatten`` of ``srcs`` by ONE :func:`devis_amd.group_norm_tokens` call, each object then bound to its
    ``[N, C, H_l, W_l]`` view of it -- when every level is a :class:`DeferredInputProjection` that is not computed yet, with one
    ``N``, ``C``, ``num_groups``, ``eps`` and dtype.  None otherwise."""
    if not srcs or not all(isinstance(s, DeferredInputProjection) and s._tensor is None for s in srcs):
        return None
    first = srcs[0]
    key = (tuple(first.x.shape[:2]), first.x.dtype, first.x.device, first.dtype, first.module.num_groups, first.module.eps,
           first.module.weight.dtype)
    for s in srcs:
        if s.x.dim() != 4 or (tuple(s.x.shape[:2]), s.x.dtype, s.x.device, s.dtype, s.module.num_groups, s.module.eps,
                              s.module.weight.dtype) != key or s.module.bias.dtype != first.module.weight.dtype:
            return None
    tokens = group_norm_tokens([s.x for s in srcs], first.module.num_groups, [s.module.weight for s in srcs],
                               [s.module.bias for s in srcs], first.module.eps, None if first.dtype == first.x.dtype else first.dtype)
    start = 0
    for s in srcs:
        H, W = s.x.shape[2:]
        s.bind(_as_map(tokens[:, start:start + H * W], (H, W)))
        start += H * W
    return tokens


def flatten_sources(srcs):
    """``cat([src.flatten(2).transpose(1, 2) for src in srcs], 1)`` -- ``prepare_data``'s ``src_flatten``: with plain tensors
    exactly that; with deferred levels of one kind :func:`fused_tokens`; a mix materialises the deferred ones first."""
    tokens = fused_tokens(srcs) if any(isinstance(s, DeferredInputProjection) for s in srcs) else None
    if tokens is not None:
        return tokens
    return torch.cat([materialized(src).flatten(2).transpose(1, 2) for src in srcs], 1)


def _feeds_next(projections, l):
    """Whether the reference feeds level ``l``'s output into projection ``l + 1``: a 3 x 3 / stride-2 projection followed by
    another one."""
    conv = projections[l][0]
    return l + 1 < len(projections) and tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (2, 2)


def patch(model):
    projections = model.input_proj
    previous = []
    for l, proj in enumerate(projections):
        if not (isinstance(proj, nn.Sequential) and len(proj) == 2 and isinstance(proj[0], nn.Conv2d) and type(proj[1]) is nn.GroupNorm):
            continue
        norm = proj[1]
        previous.append((norm, norm.__class__))
        norm.__class__ = DeferringGroupNorm
        norm.defer_output = not _feeds_next(projections, l)
    return previous


def unpatch(model, previous):
    for norm, cls in previous:
        norm.__class__ = cls
        norm.__dict__.pop("defer_output", None)
