"""ctypes binding of include/maskloss.h: the mask-loss entry points of libmsda_hip.so (the library ``_native.load()``
opens).  As in ``_mhstage``: no fallback, a failing call raises, launches go to the current stream, and the library neither
allocates nor synchronises -- outputs and workspaces are torch tensors of the caller.
"""
import ctypes

import torch

from . import _binding, _native

MASKLOSS_ABI_VERSION = 1
TARGET_U8, TARGET_SAME, TARGET_F32 = 0, 1, 2        # include/maskloss.h MASKLOSS_TARGET_*
TILE_FWD_PIXELS, TILE_FWD_SRC, TILE_BWD_ROWS, TILE_BWD_COLS, TILE_BWD_CHUNK = 0, 1, 2, 3, 4     # MASKLOSS_TILE_*
# every symbol include/maskloss.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("maskloss_version", "maskloss_last_error", "maskloss_tile", "maskloss_workspace_bytes",
                    "maskloss_forward", "maskloss_backward")

_vp, _ci, _cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


class Shape(ctypes.Structure):
    """include/maskloss.h ``maskloss_shape``."""
    _fields_ = [(name, _ci) for name in ("N", "h", "w", "H", "W")]


def _prototypes(lib):
    shape_p = ctypes.POINTER(Shape)
    lib.maskloss_tile.restype = _ci
    lib.maskloss_tile.argtypes = [_ci]
    lib.maskloss_workspace_bytes.restype = ctypes.c_longlong
    lib.maskloss_workspace_bytes.argtypes = [_ci, shape_p]
    lib.maskloss_forward.restype = _ci
    lib.maskloss_forward.argtypes = [_ci, _ci, _vp, _vp, shape_p, _cd, _cd, _vp, _vp, _vp, _vp, _vp]
    lib.maskloss_backward.restype = _ci
    lib.maskloss_backward.argtypes = [_ci, _ci, _vp, _vp, _vp, _vp, _vp, shape_p, _cd, _cd, _vp, _vp]


# load(): the library with the maskloss_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("maskloss", MASKLOSS_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


def tile(which):
    """A constant of the kernels' tiling (maskloss_tile): ``TILE_FWD_PIXELS`` consecutive destination pixels per forward
    workgroup, ``TILE_FWD_SRC`` source elements it keeps in LDS, ``TILE_BWD_ROWS`` x ``TILE_BWD_COLS`` source pixels per
    backward workgroup, ``TILE_BWD_CHUNK`` destination pixels of the derivative it holds at a time."""
    return _check(load().maskloss_tile(which), "maskloss_tile")


def target_kind(src_dtype, target_dtype):
    """include/maskloss.h ``maskloss_target`` of a target of ``target_dtype`` beside logits of ``src_dtype``: one byte per
    pixel (bool, uint8), the logits' own dtype, or float32 -- nothing else."""
    if target_dtype in (torch.bool, torch.uint8):
        return TARGET_U8
    if target_dtype == src_dtype:
        return TARGET_SAME
    if target_dtype == torch.float32:
        return TARGET_F32
    raise RuntimeError("devis_amd: mask_loss_terms: target_masks must be bool, uint8, float32 or of src_masks' dtype, got %s "
                       "beside %s" % (target_dtype, src_dtype))


def workspace_bytes(code, shape):
    """Bytes of the workspace of :func:`forward` (maskloss_workspace_bytes)."""
    return _check(load().maskloss_workspace_bytes(code, ctypes.byref(shape)), "maskloss_workspace_bytes")


def forward(code, kind, src, target, shape, alpha, gamma, workspace, focal, dice, sums):
    """maskloss_forward on the current stream: ``focal``, ``dice`` [N] and ``sums`` [N, 3], fully written."""
    with _native._on(src.device):
        rc = load().maskloss_forward(code, kind, _native._p(src), _native._p(target), ctypes.byref(shape), float(alpha),
                                     float(gamma), _native._p(workspace), _native._p(focal), _native._p(dice),
                                     _native._p(sums), _native._stream(src))
    _check(rc, "maskloss_forward")


def backward(code, kind, src, target, sums, grad_focal, grad_dice, shape, alpha, gamma, grad_src):
    """maskloss_backward on the current stream: ``grad_src`` [N, h, w], fully written."""
    with _native._on(src.device):
        rc = load().maskloss_backward(code, kind, _native._p(src), _native._p(target), _native._p(sums),
                                      _native._p(grad_focal), _native._p(grad_dice), ctypes.byref(shape), float(alpha),
                                      float(gamma), _native._p(grad_src), _native._stream(src))
    _check(rc, "maskloss_backward")
