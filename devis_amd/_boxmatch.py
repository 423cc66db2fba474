"""ctypes binding of include/boxmatch.h: the criterion's matching cost and box losses in libmsda_hip.so (the library
``_native.load()`` opens).  As in ``_maskloss``: no fallback, a failing call raises, launches go to the current stream, and the
library neither allocates nor synchronises -- outputs are torch tensors of the caller.
"""
import ctypes

import torch

from . import _binding, _native

BOXMATCH_ABI_VERSION = 1
TARGET_SAME, TARGET_F32 = 0, 1          # include/boxmatch.h BOXMATCH_TARGET_*
L1_MEAN, L1_SUM = 0, 1                  # BOXMATCH_L1_*
# every symbol include/boxmatch.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("boxmatch_version", "boxmatch_last_error", "boxmatch_cost", "boxmatch_loss_forward",
                    "boxmatch_loss_backward")

_vp, _ci, _cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


class Shape(ctypes.Structure):
    """include/boxmatch.h ``boxmatch_shape``."""
    _fields_ = [(name, _ci) for name in ("L", "F", "R", "T", "C")]


def _prototypes(lib):
    shape_p = ctypes.POINTER(Shape)
    lib.boxmatch_cost.restype = _ci
    lib.boxmatch_cost.argtypes = [_ci, _ci, _vp, _vp, _vp, _vp, shape_p, _cd, _cd, _cd, _ci, _cd, _vp, _vp, _vp]
    lib.boxmatch_loss_forward.restype = _ci
    lib.boxmatch_loss_forward.argtypes = [_ci, _ci, _vp, _vp, _ci, _vp, _vp, _vp]
    lib.boxmatch_loss_backward.restype = _ci
    lib.boxmatch_loss_backward.argtypes = [_ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _vp]


# load(): the library with the boxmatch_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("boxmatch", BOXMATCH_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


def target_kind(op, name, dtype, target_dtype):
    """include/boxmatch.h ``boxmatch_target`` of target boxes of ``target_dtype`` beside predictions of ``dtype``: the same
    dtype, or float32 beside a 16-bit one -- nothing else."""
    if target_dtype == dtype:
        return TARGET_SAME
    if target_dtype == torch.float32 and dtype in (torch.bfloat16, torch.float16):
        return TARGET_F32
    raise RuntimeError("devis_amd: %s: %s must be of the predictions' dtype (or float32 beside a 16-bit one), got %s beside %s"
                       % (op, name, target_dtype, dtype))


def cost(code, kind, logits, boxes, tgt_labels, tgt_boxes, shape, cost_class, cost_bbox, cost_giou, l1, alpha, out, status):
    """boxmatch_cost on the current stream: ``out`` [L, R, T] and ``status`` int32 [3], fully written."""
    with _native._on(logits.device):
        rc = load().boxmatch_cost(code, kind, _native._p(logits), _native._p(boxes), _native._p(tgt_labels),
                                  _native._p(tgt_boxes), ctypes.byref(shape), float(cost_class), float(cost_bbox),
                                  float(cost_giou), l1, float(alpha), _native._p(out), _native._p(status),
                                  _native._stream(logits))
    _check(rc, "boxmatch_cost")


def loss_forward(code, kind, src, tgt, N, l1, giou):
    """boxmatch_loss_forward on the current stream: ``l1`` and ``giou`` [N], fully written."""
    with _native._on(src.device):
        rc = load().boxmatch_loss_forward(code, kind, _native._p(src), _native._p(tgt), N, _native._p(l1), _native._p(giou),
                                          _native._stream(src))
    _check(rc, "boxmatch_loss_forward")


def loss_backward(code, kind, src, tgt, grad_l1, grad_giou, N, grad_src):
    """boxmatch_loss_backward on the current stream: ``grad_src`` [N, 4], fully written."""
    with _native._on(src.device):
        rc = load().boxmatch_loss_backward(code, kind, _native._p(src), _native._p(tgt), _native._p(grad_l1),
                                           _native._p(grad_giou), N, _native._p(grad_src), _native._stream(src))
    _check(rc, "boxmatch_loss_backward")
