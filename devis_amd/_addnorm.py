"""ctypes binding of include/addnorm.h: the glue between the transformer layers' GEMMs in libmsda_hip.so (the library
``_native.load()`` opens).  As in ``_labelloss``: no fallback, a failing call raises, launches go to the current stream, and the
library neither allocates nor synchronises -- outputs and the workspace are torch tensors of the caller.
"""
import ctypes

from . import _binding, _native

ADDNORM_ABI_VERSION = 1
MAX_CHANNELS = 1024                     # include/addnorm.h ADDNORM_MAX_CHANNELS
TILE_ROWS, TILE_CHANNELS = 0, 1         # include/addnorm.h ADDNORM_TILE_*
# every symbol include/addnorm.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("addnorm_version", "addnorm_last_error", "addnorm_tile", "addnorm_workspace_bytes", "addnorm_forward",
                    "addnorm_backward", "addnorm_relu_forward", "addnorm_relu_backward")

_vp, _ci, _cd, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong


class Shape(ctypes.Structure):
    """include/addnorm.h ``addnorm_shape``."""
    _fields_ = [("R", _ll), ("C", _ci)]


class Types(ctypes.Structure):
    """include/addnorm.h ``addnorm_types``: the dtype codes of x, delta, y and the parameters."""
    _fields_ = [(name, _ci) for name in ("x", "delta", "y", "param")]


def _prototypes(lib):
    shape_p, types_p = ctypes.POINTER(Shape), ctypes.POINTER(Types)
    lib.addnorm_tile.restype = _ci
    lib.addnorm_tile.argtypes = [_ci]
    lib.addnorm_workspace_bytes.restype = _ll
    lib.addnorm_workspace_bytes.argtypes = [_ci, shape_p]
    lib.addnorm_forward.restype = _ci
    lib.addnorm_forward.argtypes = [types_p, _vp, _vp, _vp, _vp, _vp, _cd, _cd, shape_p, _vp, _vp, _vp, _vp]
    lib.addnorm_backward.restype = _ci
    lib.addnorm_backward.argtypes = [types_p, _vp, _vp, _vp, _vp, _cd, _vp, _vp, _vp, shape_p, _vp, _vp, _vp, _vp, _vp, _vp]
    lib.addnorm_relu_forward.restype = _ci
    lib.addnorm_relu_forward.argtypes = [_ci, _vp, _vp, _cd, shape_p, _vp, _vp]
    lib.addnorm_relu_backward.restype = _ci
    lib.addnorm_relu_backward.argtypes = [_ci, _vp, _vp, _cd, _ll, _vp, _vp]


# load(): the library with the addnorm_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("addnorm", ADDNORM_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


_types = {}         # (x, delta, y, parameters) dtypes -> Types (read only: a layer asks for the same few on every call)


def types_of(x_dtype, delta_dtype, y_dtype, param_dtype):
    key = (x_dtype, delta_dtype, y_dtype, param_dtype)
    hit = _types.get(key)
    if hit is None:
        hit = _types[key] = Types(*(_native.dtype_code(d) for d in key))
    return hit


def tile(which=TILE_ROWS):
    """A constant of the kernels' tiling (addnorm_tile): ``TILE_ROWS`` rows per chunk of the backward's column sums -- a call of
    no more is one launch --, ``TILE_CHANNELS`` the most channels of a row."""
    return _check(load().addnorm_tile(which), "addnorm_tile")


def workspace_bytes(code, shape):
    """Bytes of the workspace of :func:`backward` (addnorm_workspace_bytes): 0 for a call of one chunk."""
    return _check(load().addnorm_workspace_bytes(code, ctypes.byref(shape)), "addnorm_workspace_bytes")


def forward(types, x, delta, weight, bias, seed, p, eps, shape, y, mean, rstd):
    """addnorm_forward on the current stream: ``y`` [R, C] fully written, ``mean`` / ``rstd`` [R] when given."""
    with _native._on(x.device):
        rc = load().addnorm_forward(ctypes.byref(types), _native._p(x), _native._p(delta), _native._p(weight), _native._p(bias),
                                    _native._p(seed), float(p), float(eps), ctypes.byref(shape), _native._p(y),
                                    _native._p(mean), _native._p(rstd), _native._stream(x))
    _check(rc, "addnorm_forward")


def backward(types, x, delta, weight, seed, p, mean, rstd, grad_y, shape, workspace, grad_x, grad_delta, grad_weight, grad_bias):
    """addnorm_backward on the current stream: the gradients that are given, fully written."""
    with _native._on(x.device):
        rc = load().addnorm_backward(ctypes.byref(types), _native._p(x), _native._p(delta), _native._p(weight), _native._p(seed),
                                     float(p), _native._p(mean), _native._p(rstd), _native._p(grad_y), ctypes.byref(shape),
                                     _native._p(workspace), _native._p(grad_x), _native._p(grad_delta), _native._p(grad_weight),
                                     _native._p(grad_bias), _native._stream(x))
    _check(rc, "addnorm_backward")


def relu_forward(code, x, seed, p, shape, y):
    """addnorm_relu_forward on the current stream: ``y`` fully written."""
    with _native._on(x.device):
        rc = load().addnorm_relu_forward(code, _native._p(x), _native._p(seed), float(p), ctypes.byref(shape), _native._p(y),
                                         _native._stream(x))
    _check(rc, "addnorm_relu_forward")


def relu_backward(code, y, grad_y, p, n, grad_x):
    """addnorm_relu_backward on the current stream: ``grad_x`` fully written."""
    with _native._on(y.device):
        rc = load().addnorm_relu_backward(code, _native._p(y), _native._p(grad_y), float(p), n, _native._p(grad_x),
                                          _native._stream(y))
    _check(rc, "addnorm_relu_backward")
