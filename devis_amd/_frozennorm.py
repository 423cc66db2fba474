"""ctypes binding of include/frozennorm.h: the glue of the ResNet backbone's blocks in libmsda_hip.so (the library
``_native.load()`` opens).  As in ``_prenorm``: no fallback, a failing call raises, launches go to the current stream, and the
library neither allocates nor synchronises -- outputs are torch tensors of the caller.
"""
import ctypes

from . import _binding, _native

FROZENNORM_ABI_VERSION = 1
NCHW, NHWC = 0, 1                       # include/frozennorm.h frozennorm_layout
NONE, PLAIN, NORMED = 0, 1, 2           # include/frozennorm.h frozennorm_residual
# every symbol include/frozennorm.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("frozennorm_version", "frozennorm_last_error", "frozennorm_pooled_size", "frozennorm_forward",
                    "frozennorm_backward", "frozennorm_pool_forward")

_vp, _ci, _cd, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong


class Shape(ctypes.Structure):
    """include/frozennorm.h ``frozennorm_shape``."""
    _fields_ = [("N", _ll)] + [(name, _ci) for name in ("C", "H", "W", "layout", "residual", "relu")]


class Types(ctypes.Structure):
    """include/frozennorm.h ``frozennorm_types``: the dtype codes of x, r and y."""
    _fields_ = [(name, _ci) for name in ("x", "r", "y")]


class Norm(ctypes.Structure):
    """include/frozennorm.h ``frozennorm_norm``: device pointers of the four float32 buffers, and eps."""
    _fields_ = [(name, _vp) for name in ("weight", "bias", "mean", "var")] + [("eps", _cd)]


def _prototypes(lib):
    shape_p, types_p, norm_p = ctypes.POINTER(Shape), ctypes.POINTER(Types), ctypes.POINTER(Norm)
    lib.frozennorm_pooled_size.restype = _ci
    lib.frozennorm_pooled_size.argtypes = [_ci]
    lib.frozennorm_forward.restype = _ci
    lib.frozennorm_forward.argtypes = [types_p, shape_p, _vp, norm_p, _vp, norm_p, _vp, _vp]
    lib.frozennorm_backward.restype = _ci
    lib.frozennorm_backward.argtypes = [types_p, shape_p, _vp, _vp, norm_p, norm_p, _vp, _vp, _vp]
    lib.frozennorm_pool_forward.restype = _ci
    lib.frozennorm_pool_forward.argtypes = [types_p, shape_p, _vp, norm_p, _vp, _vp]


# load(): the library with the frozennorm_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("frozennorm", FROZENNORM_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


_types = {}         # (x, r, y) dtypes -> Types (read only: a block asks for the same few on every call)


def types_of(x_dtype, r_dtype, y_dtype):
    key = (x_dtype, r_dtype, y_dtype)
    hit = _types.get(key)
    if hit is None:
        hit = _types[key] = Types(*(_native.dtype_code(d) for d in key))
    return hit


def _norm(norm):
    """``(weight, bias, running_mean, running_var, eps)`` of tensors (or None) -> a pointer to its ``Norm``, or None."""
    if norm is None:
        return None
    weight, bias, mean, var, eps = norm
    return ctypes.byref(Norm(_native._p(weight), _native._p(bias), _native._p(mean), _native._p(var), float(eps)))


def forward(types, shape, x, norm, r, norm_r, y):
    """frozennorm_forward on the current stream: ``y`` fully written.  ``norm`` and ``norm_r`` are
    ``(weight, bias, running_mean, running_var, eps)``."""
    with _native._on(x.device):
        rc = load().frozennorm_forward(ctypes.byref(types), ctypes.byref(shape), _native._p(x), _norm(norm), _native._p(r),
                                       _norm(norm_r), _native._p(y), _native._stream(x))
    _check(rc, "frozennorm_forward")


def backward(types, shape, grad_y, y, norm, norm_r, grad_x, grad_r):
    """frozennorm_backward on the current stream: the gradients that are given, fully written."""
    with _native._on(grad_y.device):
        rc = load().frozennorm_backward(ctypes.byref(types), ctypes.byref(shape), _native._p(grad_y), _native._p(y), _norm(norm),
                                        _norm(norm_r), _native._p(grad_x), _native._p(grad_r), _native._stream(grad_y))
    _check(rc, "frozennorm_backward")


def pool_forward(types, shape, x, norm, y):
    """frozennorm_pool_forward on the current stream: the pooled ``y`` fully written."""
    with _native._on(x.device):
        rc = load().frozennorm_pool_forward(ctypes.byref(types), ctypes.byref(shape), _native._p(x), _norm(norm), _native._p(y),
                                            _native._stream(x))
    _check(rc, "frozennorm_pool_forward")
