"""ctypes binding of include/assign.h: the linear sum assignment solver in libmsda_hip.so (the library ``_native.load()``
opens).  As in ``_boxmatch``: no fallback, a failing call raises, launches go to the current stream, and the library neither
allocates nor synchronises -- outputs are torch tensors of the caller.
"""
import ctypes

import torch

from . import _binding, _native

ASSIGN_ABI_VERSION = 1
MAX_SIDE = 1024                         # include/assign.h ASSIGN_MAX_SIDE
F32, F64 = 0, 1                         # ASSIGN_F32 / ASSIGN_F64
DTYPE_CODES = {torch.float32: F32, torch.float64: F64}
# every symbol include/assign.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("assign_version", "assign_last_error", "assign_solve")

_vp, _ci = ctypes.c_void_p, ctypes.c_int


def _prototypes(lib):
    lib.assign_solve.restype = _ci
    lib.assign_solve.argtypes = [_ci, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp]


# load(): the library with the assign_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("assign", ASSIGN_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


def solve(code, cost, L, R, T, rows, cols, status):
    """assign_solve on the current stream: ``rows`` and ``cols`` int64 [L, min(R, T)] and ``status`` int32 [2], fully
    written."""
    with _native._on(cost.device):
        rc = load().assign_solve(code, _native._p(cost), L, R, T, _native._p(rows), _native._p(cols), _native._p(status),
                                 _native._stream(cost))
    _check(rc, "assign_solve")
