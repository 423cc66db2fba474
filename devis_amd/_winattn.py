"""ctypes binding of include/winattn.h: the Swin backbone's (shifted-)window attention in libmsda_hip.so (the library
``_native.load()`` opens).  As in ``_selfattn``: no fallback, a failing call raises, launches go to the current stream, and the
library neither allocates nor synchronises -- outputs and the workspace are torch tensors of the caller.  A call returns the
number of kernel launches it enqueued.
"""
import ctypes

import torch

from . import _binding, _native

WINATTN_ABI_VERSION = 1
MAX_HEAD_DIM = 64                       # include/winattn.h WINATTN_MAX_HEAD_DIM
MAX_WINDOW = 16                         # include/winattn.h WINATTN_MAX_WINDOW
# every symbol include/winattn.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("winattn_version", "winattn_last_error", "winattn_workspace_bytes", "winattn_forward", "winattn_backward")

_vp, _ci, _cd, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong


class Shape(ctypes.Structure):
    """include/winattn.h ``winattn_shape``."""
    _fields_ = [(name, _ll) for name in ("B", "Hp", "Wp", "heads", "head_dim", "window", "shift")]


def _prototypes(lib):
    shape_p = ctypes.POINTER(Shape)
    lib.winattn_workspace_bytes.restype = _ll
    lib.winattn_workspace_bytes.argtypes = [shape_p]
    lib.winattn_forward.restype = _ci
    lib.winattn_forward.argtypes = [_ci, _ci, _vp, _vp, _cd, shape_p, _vp, _vp, _vp, _vp]
    lib.winattn_backward.restype = _ci
    lib.winattn_backward.argtypes = [_ci, _ci, _vp, _vp, _vp, _vp, _vp, _cd, shape_p, _vp, _vp, _vp, _vp]


# load(): the library with the winattn_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("winattn", WINATTN_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


def workspace_bytes(shape):
    """winattn_workspace_bytes: what ``backward`` needs beside ``grad_table`` (host arithmetic only)."""
    return _check(load().winattn_workspace_bytes(ctypes.byref(shape)), "winattn_workspace_bytes")


def forward(code, wide, qkv, table, scale, shape, out, lse, out_acc=None):
    """winattn_forward on the current stream: ``out`` [B, Hp, Wp, C] fully written, ``lse`` [B, nW, nH, N] and ``out_acc``
    [B, Hp, Wp, C] float32 -- ``out`` before its rounding -- when given.  Returns the number of launches."""
    with _native._on(qkv.device):
        rc = load().winattn_forward(code, int(wide), _native._p(qkv), _native._p(table), float(scale), ctypes.byref(shape),
                                    _native._p(out), _native._p(lse), _native._p(out_acc), _native._stream(qkv))
    return _check(rc, "winattn_forward")


def backward(code, wide, qkv, table, out, grad_out, lse, scale, shape, grad_qkv, grad_table, workspace):
    """winattn_backward on the current stream: the gradients that are given, fully written.  ``out`` is FLOAT32 whatever the
    storage dtype: the forward's ``out_acc``, or its ``out`` for float32 operands.  ``workspace`` (``workspace_bytes``) is
    needed with ``grad_table``.  Returns the number of launches: two for ``grad_qkv``, three for ``grad_table``."""
    if out.dtype != torch.float32:
        raise RuntimeError("winattn_backward: out must be float32 (the forward's out_acc), got %s" % out.dtype)
    with _native._on(qkv.device):
        rc = load().winattn_backward(code, int(wide), _native._p(qkv), _native._p(table), _native._p(out), _native._p(grad_out),
                                     _native._p(lse), float(scale), ctypes.byref(shape), _native._p(grad_qkv),
                                     _native._p(grad_table), _native._p(workspace), _native._stream(qkv))
    return _check(rc, "winattn_backward")
