"""ctypes binding of include/maskrle.h: the run-length encoder's entry points of libmsda_hip.so (the library
``_native.load()`` opens).  As in ``_maskiou``: no fallback, a failing call raises, launches go to the current stream, and the
library neither allocates nor synchronises -- the output and the workspace are torch tensors of the caller.
"""
import ctypes

from . import _binding, _native

MASKRLE_ABI_VERSION = 1
TILE_BITS_PIXELS, TILE_WORD_PIXELS, TILE_BITS_SRC, TILE_RUNS_THREADS = 0, 1, 2, 3       # include/maskrle.h MASKRLE_TILE_*
# every symbol include/maskrle.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("maskrle_version", "maskrle_last_error", "maskrle_tile", "maskrle_workspace_bytes", "maskrle_encode")

_vp, _ci = ctypes.c_void_p, ctypes.c_int


def _prototypes(lib):
    lib.maskrle_tile.restype = _ci
    lib.maskrle_tile.argtypes = [_ci]
    lib.maskrle_workspace_bytes.restype = ctypes.c_longlong
    lib.maskrle_workspace_bytes.argtypes = [_ci, _ci, _ci]
    lib.maskrle_encode.restype = _ci
    lib.maskrle_encode.argtypes = [_ci, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _vp]


# load(): the library with the maskrle_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("maskrle", MASKRLE_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


def tile(which):
    """A constant of the kernels (maskrle_tile): a workgroup of the bits pass owns ``TILE_BITS_PIXELS`` consecutive
    column-major pixels of a mask and keeps ``TILE_BITS_SRC`` source elements in LDS; a packed word of the workspace holds
    ``TILE_WORD_PIXELS`` pixels; the runs pass counts a mask with one workgroup of ``TILE_RUNS_THREADS`` threads."""
    return _check(load().maskrle_tile(which), "maskrle_tile")


def workspace_bytes(N, H, W):
    """Bytes of the workspace of :func:`encode` (maskrle_workspace_bytes)."""
    return _check(load().maskrle_workspace_bytes(N, H, W), "maskrle_workspace_bytes")


def encode(code, src, N, h, w, H, W, max_runs, workspace, runs):
    """maskrle_encode on the current stream: ``runs`` [N, 1 + max_runs] int32, fully written."""
    with _native._on(src.device):
        rc = load().maskrle_encode(code, _native._p(src), N, h, w, H, W, max_runs, _native._p(workspace), _native._p(runs),
                                   _native._stream(src))
    _check(rc, "maskrle_encode")
