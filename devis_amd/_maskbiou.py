"""ctypes binding of include/maskbiou.h: the binary mask IoU's entry points of libmsda_hip.so (the library
``_native.load()`` opens).  As in ``_maskrle``: no fallback, a failing call raises, launches go to the current stream, and the
library neither allocates nor synchronises -- the outputs and the workspace are torch tensors of the caller.
"""
import ctypes

from . import _binding, _native

MASKBIOU_ABI_VERSION = 1
TILE_BLOCK, TILE_CHUNK_WORDS, TILE_SPLIT_WORDS = 0, 1, 2       # include/maskbiou.h MASKBIOU_TILE_*
# every symbol include/maskbiou.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("maskbiou_version", "maskbiou_last_error", "maskbiou_tile", "maskbiou_workspace_bytes", "maskbiou_counts")

_vp, _ci = ctypes.c_void_p, ctypes.c_int


def _prototypes(lib):
    lib.maskbiou_tile.restype = _ci
    lib.maskbiou_tile.argtypes = [_ci]
    lib.maskbiou_workspace_bytes.restype = ctypes.c_longlong
    lib.maskbiou_workspace_bytes.argtypes = [_ci, _ci, _ci, _ci, _ci]
    lib.maskbiou_counts.restype = _ci
    lib.maskbiou_counts.argtypes = [_ci, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp]


# load(): the library with the maskbiou_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("maskbiou", MASKBIOU_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


def tile(which):
    """A constant of the kernels (maskbiou_tile): a workgroup of the pair pass owns ``TILE_BLOCK`` x ``TILE_BLOCK`` pairs and
    ``TILE_SPLIT_WORDS`` 64-pixel words of their masks, of which it stages ``TILE_CHUNK_WORDS`` per operand row in LDS at a
    time."""
    return _check(load().maskbiou_tile(which), "maskbiou_tile")


def workspace_bytes(Na, Nb, F, H, W):
    """Bytes of the workspace of :func:`counts` (maskbiou_workspace_bytes)."""
    return _check(load().maskbiou_workspace_bytes(Na, Nb, F, H, W), "maskbiou_workspace_bytes")


def counts(code, a, b, Na, Nb, F, h, w, H, W, workspace, inter, area_a, area_b):
    """maskbiou_counts on the current stream: ``inter`` [Na, Nb, F], ``area_a`` [Na, F], ``area_b`` [Nb, F] int32, fully
    written."""
    with _native._on(a.device):
        rc = load().maskbiou_counts(code, _native._p(a), _native._p(b), Na, Nb, F, h, w, H, W, _native._p(workspace),
                                    _native._p(inter), _native._p(area_a), _native._p(area_b), _native._stream(a))
    _check(rc, "maskbiou_counts")
