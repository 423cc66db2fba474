"""ctypes binding of include/labelloss.h: the criterion's label loss in libmsda_hip.so (the library ``_native.load()`` opens).
As in ``_boxmatch``: no fallback, a failing call raises, launches go to the current stream, and the library neither allocates
nor synchronises -- outputs and the workspace are torch tensors of the caller.
"""
import ctypes

from . import _binding, _native

LABELLOSS_ABI_VERSION = 1
TILE_ELEMENTS = 0                       # include/labelloss.h LABELLOSS_TILE_*
# every symbol include/labelloss.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("labelloss_version", "labelloss_last_error", "labelloss_tile", "labelloss_workspace_bytes",
                    "labelloss_forward", "labelloss_backward")

_vp, _ci, _cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


class Shape(ctypes.Structure):
    """include/labelloss.h ``labelloss_shape``."""
    _fields_ = [(name, _ci) for name in ("R", "C", "M")]


def _prototypes(lib):
    shape_p = ctypes.POINTER(Shape)
    lib.labelloss_tile.restype = _ci
    lib.labelloss_tile.argtypes = [_ci]
    lib.labelloss_workspace_bytes.restype = ctypes.c_longlong
    lib.labelloss_workspace_bytes.argtypes = [_ci, shape_p]
    lib.labelloss_forward.restype = _ci
    lib.labelloss_forward.argtypes = [_ci, _vp, _vp, _vp, _vp, shape_p, _cd, _vp, _vp, _vp, _vp, _vp]
    lib.labelloss_backward.restype = _ci
    lib.labelloss_backward.argtypes = [_ci, _vp, _vp, _vp, shape_p, _cd, _vp, _vp]


# load(): the library with the labelloss_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("labelloss", LABELLOSS_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


def tile(which=TILE_ELEMENTS):
    """A constant of the kernels' tiling (labelloss_tile): ``TILE_ELEMENTS`` logits -- whole rows -- per forward workgroup at
    most; a call of no more is one launch."""
    return _check(load().labelloss_tile(which), "labelloss_tile")


def workspace_bytes(code, shape):
    """Bytes of the workspace of :func:`forward` (labelloss_workspace_bytes): 0 for a call of one tile."""
    return _check(load().labelloss_workspace_bytes(code, ctypes.byref(shape)), "labelloss_workspace_bytes")


def forward(code, logits, rows, labels, valid, shape, alpha, workspace, target_classes, focal_sum, counts):
    """labelloss_forward on the current stream: ``target_classes`` int32 [R], ``focal_sum`` [1] and ``counts`` int32 [4],
    fully written."""
    with _native._on(logits.device):
        rc = load().labelloss_forward(code, _native._p(logits), _native._p(rows), _native._p(labels), _native._p(valid),
                                      ctypes.byref(shape), float(alpha), _native._p(workspace), _native._p(target_classes),
                                      _native._p(focal_sum), _native._p(counts), _native._stream(logits))
    _check(rc, "labelloss_forward")


def backward(code, logits, target_classes, grad_sum, shape, alpha, grad_logits):
    """labelloss_backward on the current stream: ``grad_logits`` [R, C], fully written."""
    with _native._on(logits.device):
        rc = load().labelloss_backward(code, _native._p(logits), _native._p(target_classes), _native._p(grad_sum),
                                       ctypes.byref(shape), float(alpha), _native._p(grad_logits), _native._stream(logits))
    _check(rc, "labelloss_backward")
