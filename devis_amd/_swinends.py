"""ctypes binding of include/swinends.h: the two ends of the Swin backbone in libmsda_hip.so (the library ``_native.load()``
opens) -- the patch embedding with its norm in token order, and the per-stage output norm in NCHW.  As in ``_prenorm``: no
fallback, a failing call raises, launches go to the current stream, and the library neither allocates nor synchronises --
outputs and the workspaces are torch tensors of the caller.
"""
import ctypes

from . import _binding, _native

SWINENDS_ABI_VERSION = 1
MAX_PATCH, MAX_EMBED, MAX_CHANNELS = 192, 1024, 3072        # include/swinends.h SWINENDS_MAX_*
TILE_TOKENS, TILE_EMBED_CHUNK, TILE_MAX_PATCH, TILE_MAX_EMBED, TILE_MAX_CHANNELS = 0, 1, 2, 3, 4     # SWINENDS_TILE_*
# every symbol include/swinends.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("swinends_version", "swinends_last_error", "swinends_tile", "swinends_embed_tokens",
                    "swinends_embed_workspace_bytes", "swinends_embed_forward", "swinends_embed_backward",
                    "swinends_map_workspace_bytes", "swinends_map_forward", "swinends_map_backward")

_vp, _ci, _cd, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong


class EmbedShape(ctypes.Structure):
    """include/swinends.h ``swinends_embed_shape``."""
    _fields_ = [("B", _ll)] + [(name, _ci) for name in ("Cin", "H", "W", "p", "C")]


class EmbedTypes(ctypes.Structure):
    """include/swinends.h ``swinends_embed_types``: the dtype codes of the image, the parameters and the tokens."""
    _fields_ = [(name, _ci) for name in ("image", "param", "y")]


class MapShape(ctypes.Structure):
    """include/swinends.h ``swinends_map_shape``."""
    _fields_ = [("B", _ll)] + [(name, _ci) for name in ("H", "W", "C")]


class MapTypes(ctypes.Structure):
    """include/swinends.h ``swinends_map_types``: the dtype codes of x, y and the parameters."""
    _fields_ = [(name, _ci) for name in ("x", "y", "param")]


def _prototypes(lib):
    es, et, ms, mt = (ctypes.POINTER(c) for c in (EmbedShape, EmbedTypes, MapShape, MapTypes))
    lib.swinends_tile.restype = _ci
    lib.swinends_tile.argtypes = [_ci]
    lib.swinends_embed_tokens.restype = _ll
    lib.swinends_embed_tokens.argtypes = [es]
    lib.swinends_embed_workspace_bytes.restype = _ll
    lib.swinends_embed_workspace_bytes.argtypes = [es, _ci]
    lib.swinends_embed_forward.restype = _ci
    lib.swinends_embed_forward.argtypes = [et, _vp, _vp, _vp, _vp, _vp, _cd, es, _vp, _vp, _vp, _vp]
    lib.swinends_embed_backward.restype = _ci
    lib.swinends_embed_backward.argtypes = [et, _vp, _vp, _vp, _vp, _vp, _vp, _vp, es, _vp, _vp, _vp, _vp, _vp, _vp]
    lib.swinends_map_workspace_bytes.restype = _ll
    lib.swinends_map_workspace_bytes.argtypes = [ms]
    lib.swinends_map_forward.restype = _ci
    lib.swinends_map_forward.argtypes = [mt, _vp, _vp, _vp, _cd, ms, _vp, _vp, _vp, _vp]
    lib.swinends_map_backward.restype = _ci
    lib.swinends_map_backward.argtypes = [mt, _vp, _vp, _vp, _vp, _vp, ms, _vp, _vp, _vp, _vp, _vp]


# load(): the library with the swinends_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("swinends", SWINENDS_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


def embed_types_of(image_dtype, param_dtype, y_dtype):
    return EmbedTypes(*(_native.dtype_code(d) for d in (image_dtype, param_dtype, y_dtype)))


def map_types_of(x_dtype, y_dtype, param_dtype):
    return MapTypes(*(_native.dtype_code(d) for d in (x_dtype, y_dtype, param_dtype)))


def tile(which=TILE_TOKENS):
    """A constant of the kernels' tiling (swinends_tile): ``TILE_TOKENS`` tokens of a workgroup's tile, ``TILE_EMBED_CHUNK``
    tokens per chunk of the embedding backward's sums, and the three limits."""
    return _check(load().swinends_tile(which), "swinends_tile")


def embed_tokens(shape):
    """The tokens of a shape (swinends_embed_tokens)."""
    return _check(load().swinends_embed_tokens(ctypes.byref(shape)), "swinends_embed_tokens")


def embed_workspace_bytes(shape, want_weight):
    """Bytes of the workspace of :func:`embed_backward` (swinends_embed_workspace_bytes)."""
    return _check(load().swinends_embed_workspace_bytes(ctypes.byref(shape), int(bool(want_weight))), "swinends_embed_workspace_bytes")


def map_workspace_bytes(shape):
    """Bytes of the workspace of :func:`map_backward` when a parameter gradient is asked for (swinends_map_workspace_bytes)."""
    return _check(load().swinends_map_workspace_bytes(ctypes.byref(shape)), "swinends_map_workspace_bytes")


def embed_forward(types, image, proj_weight, proj_bias, norm_weight, norm_bias, eps, shape, tokens, mean, rstd):
    """swinends_embed_forward on the current stream: ``tokens`` fully written, ``mean`` / ``rstd`` when given."""
    p = _native._p
    with _native._on(image.device):
        rc = load().swinends_embed_forward(ctypes.byref(types), p(image), p(proj_weight), p(proj_bias), p(norm_weight), p(norm_bias),
                                           float(eps), ctypes.byref(shape), p(tokens), p(mean), p(rstd), _native._stream(image))
    _check(rc, "swinends_embed_forward")


def embed_backward(types, image, proj_weight, proj_bias, norm_weight, mean, rstd, grad_tokens, shape, workspace, grad_proj_weight,
                   grad_proj_bias, grad_norm_weight, grad_norm_bias):
    """swinends_embed_backward on the current stream: the gradients that are given, fully written."""
    p = _native._p
    with _native._on(image.device):
        rc = load().swinends_embed_backward(ctypes.byref(types), p(image), p(proj_weight), p(proj_bias), p(norm_weight), p(mean),
                                            p(rstd), p(grad_tokens), ctypes.byref(shape), p(workspace), p(grad_proj_weight),
                                            p(grad_proj_bias), p(grad_norm_weight), p(grad_norm_bias), _native._stream(image))
    _check(rc, "swinends_embed_backward")


def map_forward(types, x, weight, bias, eps, shape, y, mean, rstd):
    """swinends_map_forward on the current stream: ``y [B, C, H, W]`` fully written, ``mean`` / ``rstd`` when given."""
    p = _native._p
    with _native._on(x.device):
        rc = load().swinends_map_forward(ctypes.byref(types), p(x), p(weight), p(bias), float(eps), ctypes.byref(shape), p(y),
                                         p(mean), p(rstd), _native._stream(x))
    _check(rc, "swinends_map_forward")


def map_backward(types, x, weight, mean, rstd, grad_y, shape, workspace, grad_x, grad_weight, grad_bias):
    """swinends_map_backward on the current stream: the gradients that are given, fully written."""
    p = _native._p
    with _native._on(x.device):
        rc = load().swinends_map_backward(ctypes.byref(types), p(x), p(weight), p(mean), p(rstd), p(grad_y), ctypes.byref(shape),
                                          p(workspace), p(grad_x), p(grad_weight), p(grad_bias), _native._stream(x))
    _check(rc, "swinends_map_backward")
