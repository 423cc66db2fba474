"""ctypes binding of include/posembed.h: the encoder's positional input in libmsda_hip.so (the library ``_native.load()``
opens).  As in ``_labelloss``: no fallback, a failing call raises, launches go to the current stream, and the library neither
allocates nor synchronises -- outputs and the workspace are torch tensors of the caller.
"""
import ctypes

from . import _binding, _native

POSEMBED_ABI_VERSION = 1
MAX_LEVELS = 8                                              # include/posembed.h POSEMBED_MAX_LEVELS
TILE_TOKENS, TILE_CHANNELS, TILE_PIXELS = 0, 1, 2           # POSEMBED_TILE_*
WS_COUNTS, WS_BACKWARD = 0, 1                               # POSEMBED_WS_*
NO_ROUNDING = -1                                            # POSEMBED_NO_ROUNDING
# every symbol include/posembed.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("posembed_version", "posembed_last_error", "posembed_tile", "posembed_workspace_bytes", "posembed_counts",
                    "posembed_write_flat", "posembed_write_nchw", "posembed_backward")

_vp, _ci, _cf, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong


class Shape(ctypes.Structure):
    """include/posembed.h ``posembed_shape``."""
    _fields_ = [("N", _ci), ("L", _ci), ("C", _ci), ("H", _ci * MAX_LEVELS), ("W", _ci * MAX_LEVELS)]


class Masks(ctypes.Structure):
    """include/posembed.h ``posembed_masks``."""
    _fields_ = [("ptr", _vp * MAX_LEVELS), ("sn", _ll * MAX_LEVELS), ("sy", _ll * MAX_LEVELS), ("sx", _ll * MAX_LEVELS)]


def shape_of(N, sizes, C):
    """The ``posembed_shape`` of ``N`` frames, levels ``sizes = [(H, W), ...]`` and ``C`` channels."""
    if not 1 <= len(sizes) <= MAX_LEVELS:
        raise RuntimeError("devis_amd: position embedding takes 1 to %d levels, got %d" % (MAX_LEVELS, len(sizes)))
    s = Shape(N=N, L=len(sizes), C=C)
    for l, (h, w) in enumerate(sizes):
        s.H[l], s.W[l] = h, w
    return s


def masks_of(masks):
    """The ``posembed_masks`` of bool / uint8 tensors [N, H, W] as they lie (any strides)."""
    m = Masks()
    for l, t in enumerate(masks):
        m.ptr[l] = t.data_ptr()
        m.sn[l], m.sy[l], m.sx[l] = t.stride()
    return m


def _prototypes(lib):
    shape_p = ctypes.POINTER(Shape)
    lib.posembed_tile.restype = _ci
    lib.posembed_tile.argtypes = [_ci]
    lib.posembed_workspace_bytes.restype = _ll
    lib.posembed_workspace_bytes.argtypes = [_ci, shape_p]
    lib.posembed_counts.restype = _ci
    lib.posembed_counts.argtypes = [ctypes.POINTER(Masks), shape_p, _vp, _vp, _vp, _vp]
    lib.posembed_write_flat.restype = _ci
    lib.posembed_write_flat.argtypes = [_ci, _vp, shape_p, _vp, _vp, _vp, _ci, _cf, _ci, _vp, _vp]
    lib.posembed_write_nchw.restype = _ci
    lib.posembed_write_nchw.argtypes = [_ci, _vp, shape_p, _vp, _ci, _cf, _vp, _vp]
    lib.posembed_backward.restype = _ci
    lib.posembed_backward.argtypes = [_ci, _vp, shape_p, _vp, _vp, _vp, _vp]


# load(): the library with the posembed_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("posembed", POSEMBED_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


def tile(which=TILE_TOKENS):
    """A constant of the kernels' tiling (posembed_tile): ``TILE_TOKENS`` tokens of one level and frame and ``TILE_CHANNELS``
    channels per workgroup of the backward's partial pass; ``TILE_PIXELS`` pixels of a row per ballot of the counts pass."""
    return _check(load().posembed_tile(which), "posembed_tile")


def workspace_bytes(which, shape):
    """Bytes of the workspace of :func:`counts` (``WS_COUNTS``) or :func:`backward` (``WS_BACKWARD``)."""
    return _check(load().posembed_workspace_bytes(which, ctypes.byref(shape)), "posembed_workspace_bytes")


def counts(masks, shape, workspace, mask_flatten, valid_ratios):
    """posembed_counts on the current stream: the counts in ``workspace``, ``mask_flatten`` [N, S] and ``valid_ratios``
    [N, L, 2] (either may be None)."""
    with _native._on(workspace.device):
        rc = load().posembed_counts(ctypes.byref(masks_of(masks)), ctypes.byref(shape), _native._p(workspace),
                                    _native._p(mask_flatten), _native._p(valid_ratios), _native._stream(workspace))
    _check(rc, "posembed_counts")


def write_flat(code, workspace, shape, dim_t, level_embed, temporal_embed, normalize, scale, round_code, pos):
    """posembed_write_flat on the current stream: ``pos`` [N, S, C], fully written."""
    with _native._on(pos.device):
        rc = load().posembed_write_flat(code, _native._p(workspace), ctypes.byref(shape), _native._p(dim_t),
                                        _native._p(level_embed), _native._p(temporal_embed), int(bool(normalize)), float(scale),
                                        round_code, _native._p(pos), _native._stream(pos))
    _check(rc, "posembed_write_flat")


def write_nchw(code, workspace, shape, dim_t, normalize, scale, pos):
    """posembed_write_nchw on the current stream: ``pos`` [N, C, H, W], fully written."""
    with _native._on(pos.device):
        rc = load().posembed_write_nchw(code, _native._p(workspace), ctypes.byref(shape), _native._p(dim_t),
                                        int(bool(normalize)), float(scale), _native._p(pos), _native._stream(pos))
    _check(rc, "posembed_write_nchw")


def backward(code, grad, shape, workspace, grad_level_embed, grad_temporal_embed):
    """posembed_backward on the current stream: the gradients that are not None, fully written."""
    with _native._on(grad.device):
        rc = load().posembed_backward(code, _native._p(grad), ctypes.byref(shape), _native._p(workspace),
                                      _native._p(grad_level_embed), _native._p(grad_temporal_embed), _native._stream(grad))
    _check(rc, "posembed_backward")
