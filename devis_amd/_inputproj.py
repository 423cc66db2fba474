"""ctypes binding of include/inputproj.h: the GroupNorm of the encoder's input projections written as flat tokens, in
libmsda_hip.so (the library ``_native.load()`` opens).  As in ``_swinends``: no fallback, a failing call raises, launches go to
the current stream, and the library neither allocates nor synchronises -- outputs and the workspaces are torch tensors of the
caller.
"""
import ctypes

from . import _binding, _native

INPUTPROJ_ABI_VERSION = 1
MAX_LEVELS, MAX_CHANNELS = 8, 1024                          # include/inputproj.h INPUTPROJ_MAX_*
TILE_PIXELS, TILE_CHANNELS, TILE_STAT_CHUNK, TILE_SUM_CHUNK, TILE_MAX_LEVELS, TILE_MAX_CHANNELS = 0, 1, 2, 3, 4, 5   # INPUTPROJ_TILE_*
# every symbol include/inputproj.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("inputproj_version", "inputproj_last_error", "inputproj_tile", "inputproj_tokens",
                    "inputproj_forward_workspace_bytes", "inputproj_backward_workspace_bytes", "inputproj_forward",
                    "inputproj_backward")

_vp, _ci, _cd, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong


class Shape(ctypes.Structure):
    """include/inputproj.h ``inputproj_shape``."""
    _fields_ = [("N", _ll), ("C", _ci), ("G", _ci), ("L", _ci), ("H", _ci * MAX_LEVELS), ("W", _ci * MAX_LEVELS)]


class Types(ctypes.Structure):
    """include/inputproj.h ``inputproj_types``: the dtype codes of the maps, the parameters and the tokens."""
    _fields_ = [(name, _ci) for name in ("x", "param", "y")]


class Levels(ctypes.Structure):
    """include/inputproj.h ``inputproj_levels``: one device pointer per level."""
    _fields_ = [("p", _vp * MAX_LEVELS)]


def _prototypes(lib):
    sh, ty, lv = (ctypes.POINTER(c) for c in (Shape, Types, Levels))
    lib.inputproj_tile.restype = _ci
    lib.inputproj_tile.argtypes = [_ci]
    for name in ("inputproj_tokens", "inputproj_forward_workspace_bytes", "inputproj_backward_workspace_bytes"):
        getattr(lib, name).restype = _ll
        getattr(lib, name).argtypes = [sh]
    lib.inputproj_forward.restype = _ci
    lib.inputproj_forward.argtypes = [ty, lv, lv, lv, _cd, sh, _vp, _vp, _vp, _vp, _vp]
    lib.inputproj_backward.restype = _ci
    lib.inputproj_backward.argtypes = [ty, lv, lv, _vp, _vp, _vp, sh, _vp, lv, lv, lv, _vp]


# load(): the library with the inputproj_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("inputproj", INPUTPROJ_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


def shape_of(N, C, G, sizes):
    """The ``inputproj_shape`` of ``N`` frames, ``C`` channels in ``G`` groups and the levels ``sizes = [(H, W), ...]``."""
    if not 1 <= len(sizes) <= MAX_LEVELS:
        raise ValueError("devis_amd: 1 to %d levels, got %d" % (MAX_LEVELS, len(sizes)))
    shape = Shape(N, C, G, len(sizes))
    for l, (h, w) in enumerate(sizes):
        shape.H[l], shape.W[l] = h, w
    return shape


def types_of(x_dtype, param_dtype, y_dtype):
    return Types(*(_native.dtype_code(d) for d in (x_dtype, param_dtype, y_dtype)))


def levels_of(tensors):
    """The ``inputproj_levels`` of a sequence of tensors (None: a NULL entry)."""
    table = Levels()
    for l, t in enumerate(tensors):
        table.p[l] = _native._p(t)
    return table


def tile(which=TILE_PIXELS):
    """A constant of the kernels' tiling (inputproj_tile): pixels and channels of a tile, elements of a statistics chunk, pixels
    of a chunk of the backward's sums, and the two limits."""
    return _check(load().inputproj_tile(which), "inputproj_tile")


def tokens(shape):
    """The tokens of a frame (inputproj_tokens)."""
    return _check(load().inputproj_tokens(ctypes.byref(shape)), "inputproj_tokens")


def forward_workspace_bytes(shape):
    """Bytes of the workspace of :func:`forward`: 0 when every group is one statistics chunk."""
    return _check(load().inputproj_forward_workspace_bytes(ctypes.byref(shape)), "inputproj_forward_workspace_bytes")


def backward_workspace_bytes(shape):
    """Bytes of the workspace of :func:`backward`."""
    return _check(load().inputproj_backward_workspace_bytes(ctypes.byref(shape)), "inputproj_backward_workspace_bytes")


def forward(types, xs, weights, biases, eps, shape, workspace, tokens_out, mean, rstd):
    """inputproj_forward on the current stream: ``tokens_out``, ``mean`` and ``rstd`` fully written."""
    p = _native._p
    with _native._on(tokens_out.device):
        rc = load().inputproj_forward(ctypes.byref(types), ctypes.byref(levels_of(xs)), ctypes.byref(levels_of(weights)),
                                      ctypes.byref(levels_of(biases)), float(eps), ctypes.byref(shape), p(workspace), p(tokens_out),
                                      p(mean), p(rstd), _native._stream(tokens_out))
    _check(rc, "inputproj_forward")


def backward(types, xs, weights, mean, rstd, grad_tokens, shape, workspace, grad_xs, grad_weights, grad_biases):
    """inputproj_backward on the current stream: the gradients that are given (not None), fully written."""
    p = _native._p
    with _native._on(grad_tokens.device):
        rc = load().inputproj_backward(ctypes.byref(types), ctypes.byref(levels_of(xs)), ctypes.byref(levels_of(weights)), p(mean),
                                       p(rstd), p(grad_tokens), ctypes.byref(shape), p(workspace), ctypes.byref(levels_of(grad_xs)),
                                       ctypes.byref(levels_of(grad_weights)), ctypes.byref(levels_of(grad_biases)),
                                       _native._stream(grad_tokens))
    _check(rc, "inputproj_backward")
