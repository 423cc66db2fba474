"""ctypes binding of include/mhstage.h: the mask-head-stage entry points of libmsda_hip.so (the library ``_native.load()``
opens).  As in ``_attmap``: no fallback, a failing call raises, launches go to the current stream, and the library neither
allocates nor synchronises -- outputs and workspaces are torch tensors of the caller.
"""
import ctypes

import torch

from . import _binding, _native

MHSTAGE_ABI_VERSION = 1
GRAD_X, GRAD_WEIGHT, GRAD_BIAS, GRAD_SKIP = 1, 2, 4, 8      # include/mhstage.h MHSTAGE_GRAD_*
GRAD_ALL = GRAD_X | GRAD_WEIGHT | GRAD_BIAS | GRAD_SKIP
TILE_STAT, TILE_APPLY_PIXELS, TILE_APPLY_CHANNELS, TILE_BWD_PIXELS = 0, 1, 2, 3     # MHSTAGE_TILE_*
# every symbol include/mhstage.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("mhstage_version", "mhstage_last_error", "mhstage_tile", "mhstage_workspace_bytes", "mhstage_forward",
                    "mhstage_backward")

_vp, _ci = ctypes.c_void_p, ctypes.c_int


class Shape(ctypes.Structure):
    """include/mhstage.h ``mhstage_shape``."""
    _fields_ = [(name, _ci) for name in ("N", "F", "C", "G", "E", "h", "w", "H", "W")]


def _prototypes(lib):
    shape_p = ctypes.POINTER(Shape)
    lib.mhstage_tile.restype = _ci
    lib.mhstage_tile.argtypes = [_ci]
    lib.mhstage_workspace_bytes.restype = ctypes.c_longlong
    lib.mhstage_workspace_bytes.argtypes = [_ci, shape_p]
    lib.mhstage_forward.restype = _ci
    lib.mhstage_forward.argtypes = [_ci, _ci, _ci, _ci, _vp, _vp, _vp, ctypes.c_double, _vp, _vp, _ci, _vp, shape_p,
                                    _vp, _vp, _vp, _vp, _vp]
    lib.mhstage_backward.restype = _ci
    lib.mhstage_backward.argtypes = [_ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _ci, shape_p,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _vp]


# load(): the library with the mhstage_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("mhstage", MHSTAGE_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


def tile(which):
    """A constant of the kernels' tiling (mhstage_tile): ``TILE_STAT`` elements of a group block per statistics tile,
    ``TILE_APPLY_PIXELS`` x ``TILE_APPLY_CHANNELS`` per apply workgroup, ``TILE_BWD_PIXELS`` source pixels per workgroup
    of backward pass 1."""
    return _check(load().mhstage_tile(which), "mhstage_tile")


def wide_dtype(dtype, requested, what):
    """The storage type of a tensor that may be float32 beside 16-bit ``dtype``: ``dtype`` itself (also for None), or
    float32 beside bfloat16 / float16 -- nothing else."""
    if requested is None or requested == dtype:
        return dtype
    if requested == torch.float32 and dtype in (torch.bfloat16, torch.float16):
        return requested
    raise RuntimeError("devis_amd: mask_head_stage: %s must have x's dtype (or float32 beside a 16-bit x), got %s beside %s"
                       % (what, requested, dtype))


def src_index(d, size_in, size_out):
    """include/mhstage.h ``src``: PyTorch's mode="nearest" source index of destination index ``d`` along an axis that goes
    from ``size_in`` to ``size_out``, in float32 as the kernels evaluate it."""
    f32 = torch.float32
    scale = torch.tensor(float(size_in), dtype=f32) / torch.tensor(float(size_out), dtype=f32)
    return min(int(torch.floor(torch.tensor(float(d), dtype=f32) * scale)), size_in - 1)


def workspace_bytes(code, shape):
    """Bytes of the workspace of :func:`forward` and :func:`backward` (mhstage_workspace_bytes)."""
    return _check(load().mhstage_workspace_bytes(code, ctypes.byref(shape)), "mhstage_workspace_bytes")


def _is64(index):
    return int(index is not None and index.dtype == torch.int64)


def forward(code, param_wide, extra_wide, out_wide, x, weight, bias, eps, skip, skip_index, extra, shape, workspace, mean,
            rstd, out):
    """mhstage_forward on the current stream: ``mean``, ``rstd`` [N, G] and ``out`` (channels-last memory), fully
    written."""
    with _native._on(x.device):
        rc = load().mhstage_forward(code, int(param_wide), int(extra_wide), int(out_wide), _native._p(x), _native._p(weight),
                                    _native._p(bias), float(eps), _native._p(skip), _native._p(skip_index), _is64(skip_index),
                                    _native._p(extra), ctypes.byref(shape), _native._p(workspace), _native._p(mean),
                                    _native._p(rstd), _native._p(out), _native._stream(x))
    _check(rc, "mhstage_forward")


def backward(grads, code, param_wide, out_wide, x, weight, bias, mean, rstd, skip_index, grad_out, channels_last, shape,
             workspace, dy, grad_x, grad_weight, grad_bias, grad_skip):
    """mhstage_backward on the current stream: the gradients in ``grads``, each fully written."""
    with _native._on(grad_out.device):
        rc = load().mhstage_backward(grads, code, int(param_wide), int(out_wide), _native._p(x), _native._p(weight),
                                     _native._p(bias), _native._p(mean), _native._p(rstd), _native._p(skip_index),
                                     _is64(skip_index), _native._p(grad_out), int(channels_last), ctypes.byref(shape),
                                     _native._p(workspace), _native._p(dy), _native._p(grad_x), _native._p(grad_weight),
                                     _native._p(grad_bias), _native._p(grad_skip), _native._stream(grad_out))
    _check(rc, "mhstage_backward")
