"""ctypes binding of include/prenorm.h: the glue of the Swin backbone's blocks in libmsda_hip.so (the library
``_native.load()`` opens).  As in ``_addnorm``: no fallback, a failing call raises, launches go to the current stream, and the
library neither allocates nor synchronises -- outputs and the workspace are torch tensors of the caller.
"""
import ctypes

from . import _binding, _native

PRENORM_ABI_VERSION = 1
MAX_CHANNELS = 3072                     # include/prenorm.h PRENORM_MAX_CHANNELS
TILE_ROWS, TILE_CHANNELS = 0, 1         # include/prenorm.h PRENORM_TILE_*
PLAIN, RESIDUAL, MERGE = 0, 1, 2        # include/prenorm.h prenorm_source
TOKENS, MAP = 0, 1                      # include/prenorm.h prenorm_dest
# every symbol include/prenorm.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("prenorm_version", "prenorm_last_error", "prenorm_tile", "prenorm_rows", "prenorm_workspace_bytes",
                    "prenorm_forward", "prenorm_backward")

_vp, _ci, _cd, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong


class Shape(ctypes.Structure):
    """include/prenorm.h ``prenorm_shape``."""
    _fields_ = [("B", _ll)] + [(name, _ci) for name in ("H", "W", "C", "Hp", "Wp", "source", "dest")]


class Types(ctypes.Structure):
    """include/prenorm.h ``prenorm_types``: the dtype codes of x, delta, y and the parameters."""
    _fields_ = [(name, _ci) for name in ("x", "delta", "y", "param")]


def _prototypes(lib):
    shape_p, types_p = ctypes.POINTER(Shape), ctypes.POINTER(Types)
    lib.prenorm_tile.restype = _ci
    lib.prenorm_tile.argtypes = [_ci]
    lib.prenorm_rows.restype = _ll
    lib.prenorm_rows.argtypes = [shape_p]
    lib.prenorm_workspace_bytes.restype = _ll
    lib.prenorm_workspace_bytes.argtypes = [shape_p]
    lib.prenorm_forward.restype = _ci
    lib.prenorm_forward.argtypes = [types_p, _vp, _vp, _vp, _vp, _vp, _cd, shape_p, _vp, _vp, _vp, _vp, _vp]
    lib.prenorm_backward.restype = _ci
    lib.prenorm_backward.argtypes = [types_p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, shape_p, _vp, _vp, _vp, _vp, _vp, _vp]


# load(): the library with the prenorm_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("prenorm", PRENORM_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


_types = {}         # (x, delta, y, parameters) dtypes -> Types (read only: a block asks for the same few on every call)


def types_of(x_dtype, delta_dtype, y_dtype, param_dtype):
    key = (x_dtype, delta_dtype, y_dtype, param_dtype)
    hit = _types.get(key)
    if hit is None:
        hit = _types[key] = Types(*(_native.dtype_code(d) for d in key))
    return hit


def tile(which=TILE_ROWS):
    """A constant of the kernels' tiling (prenorm_tile): ``TILE_ROWS`` rows per chunk of the backward's column sums -- a call of
    no more is one launch --, ``TILE_CHANNELS`` the most channels of a row."""
    return _check(load().prenorm_tile(which), "prenorm_tile")


def rows(shape):
    """The rows of a shape (prenorm_rows)."""
    return _check(load().prenorm_rows(ctypes.byref(shape)), "prenorm_rows")


def workspace_bytes(shape):
    """Bytes of the workspace of :func:`backward` (prenorm_workspace_bytes): 0 for a call of one chunk."""
    return _check(load().prenorm_workspace_bytes(ctypes.byref(shape)), "prenorm_workspace_bytes")


def forward(types, x, delta, keep, weight, bias, eps, shape, s, y, mean, rstd):
    """prenorm_forward on the current stream: ``y`` fully written (a map's padding as 0), ``s`` in the residual form,
    ``mean`` / ``rstd`` [R] when given."""
    with _native._on(x.device):
        rc = load().prenorm_forward(ctypes.byref(types), _native._p(x), _native._p(delta), _native._p(keep), _native._p(weight),
                                    _native._p(bias), float(eps), ctypes.byref(shape), _native._p(s), _native._p(y),
                                    _native._p(mean), _native._p(rstd), _native._stream(x))
    _check(rc, "prenorm_forward")


def backward(types, x, keep, weight, mean, rstd, grad_y, grad_s, shape, workspace, grad_x, grad_delta, grad_weight, grad_bias):
    """prenorm_backward on the current stream: the gradients that are given, fully written.  ``x`` is what the rows are read
    from: the forward's ``s`` in the residual form."""
    with _native._on(x.device):
        rc = load().prenorm_backward(ctypes.byref(types), _native._p(x), _native._p(keep), _native._p(weight), _native._p(mean),
                                     _native._p(rstd), _native._p(grad_y), _native._p(grad_s), ctypes.byref(shape),
                                     _native._p(workspace), _native._p(grad_x), _native._p(grad_delta), _native._p(grad_weight),
                                     _native._p(grad_bias), _native._stream(x))
    _check(rc, "prenorm_backward")
