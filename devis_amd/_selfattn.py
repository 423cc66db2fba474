"""ctypes binding of include/selfattn.h: the decoder's query self-attention in libmsda_hip.so (the library ``_native.load()``
opens).  As in ``_addnorm``: no fallback, a failing call raises, launches go to the current stream, and the library neither
allocates nor synchronises -- outputs are torch tensors of the caller.  A call returns the number of kernel launches it enqueued.
"""
import ctypes

import torch

from . import _binding, _native

SELFATTN_ABI_VERSION = 2
MAX_HEAD_DIM = 64                       # include/selfattn.h SELFATTN_MAX_HEAD_DIM
# every symbol include/selfattn.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("selfattn_version", "selfattn_last_error", "selfattn_forward", "selfattn_backward")

_vp, _ci, _cd, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong


class Shape(ctypes.Structure):
    """include/selfattn.h ``selfattn_shape``."""
    _fields_ = [(name, _ll) for name in ("L", "S", "N", "E", "H")]


class View(ctypes.Structure):
    """include/selfattn.h ``selfattn_view``: the strides of a [sequence, batch, channel] operand, in elements."""
    _fields_ = [(name, _ll) for name in ("seq", "batch", "channel")]


def _prototypes(lib):
    shape_p, view_p = ctypes.POINTER(Shape), ctypes.POINTER(View)
    lib.selfattn_forward.restype = _ci
    lib.selfattn_forward.argtypes = [_ci, _vp, view_p, _vp, view_p, _vp, view_p, _vp, _cd, shape_p, _vp, _vp, _vp, _vp]
    lib.selfattn_backward.restype = _ci
    lib.selfattn_backward.argtypes = [_ci, _vp, view_p, _vp, view_p, _vp, view_p, _vp, _vp, _vp, _vp, _cd, shape_p, _vp, _vp,
                                      _vp, _vp]


# load(): the library with the selfattn_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("selfattn", SELFATTN_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


def view_of(t):
    """The ``View`` of a [sequence, batch, channel] tensor."""
    return View(t.stride(0), t.stride(1), t.stride(2))


def forward(code, q, k, v, seed, p, shape, out, lse, out_acc=None):
    """selfattn_forward on the current stream: ``out`` [L, N, E] fully written, ``lse`` [N * H, L] and ``out_acc`` [L, N, E]
    float32 -- ``out`` before its rounding -- when given.  ``q``, ``k`` and ``v`` are passed with their strides.  Returns the
    number of launches."""
    with _native._on(q.device):
        rc = load().selfattn_forward(code, _native._p(q), ctypes.byref(view_of(q)), _native._p(k), ctypes.byref(view_of(k)),
                                     _native._p(v), ctypes.byref(view_of(v)), _native._p(seed), float(p), ctypes.byref(shape),
                                     _native._p(out), _native._p(lse), _native._p(out_acc), _native._stream(q))
    return _check(rc, "selfattn_forward")


def backward(code, q, k, v, out, grad_out, lse, seed, p, shape, grad_q, grad_k, grad_v):
    """selfattn_backward on the current stream: the gradients that are given, fully written.  ``out`` is FLOAT32 whatever the
    storage dtype: the forward's ``out_acc``, or its ``out`` for float32 operands.  Returns the number of launches: one for
    ``grad_q``, one for ``grad_k`` and / or ``grad_v``."""
    if out.dtype != torch.float32:
        raise RuntimeError("selfattn_backward: out must be float32 (the forward's out_acc), got %s" % out.dtype)
    with _native._on(q.device):
        rc = load().selfattn_backward(code, _native._p(q), ctypes.byref(view_of(q)), _native._p(k), ctypes.byref(view_of(k)),
                                      _native._p(v), ctypes.byref(view_of(v)), _native._p(out), _native._p(grad_out),
                                      _native._p(lse), _native._p(seed), float(p), ctypes.byref(shape), _native._p(grad_q),
                                      _native._p(grad_k), _native._p(grad_v), _native._stream(q))
    return _check(rc, "selfattn_backward")
