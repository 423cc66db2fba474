"""ctypes binding of include/maskiou.h: the clip-stitching entry points of libmsda_hip.so (the library ``_native.load()``
opens).  As in ``_maskloss``: no fallback, a failing call raises, launches go to the current stream, and the library neither
allocates nor synchronises -- outputs and workspaces are torch tensors of the caller.
"""
import ctypes

from . import _binding, _native

MASKIOU_ABI_VERSION = 1
VOLUME, FRAME = 0, 1                    # include/maskiou.h MASKIOU_VOLUME / MASKIOU_FRAME
ROW_MAJOR, COL_MAJOR = 0, 1             # MASKIOU_ROW_MAJOR / MASKIOU_COL_MAJOR
TILE_BLOCK, TILE_ROWS, TILE_COLS, TILE_SPLIT_TILES, TILE_MAX_SPLITS, TILE_BIN_PIXELS, TILE_BIN_SRC = 0, 1, 2, 3, 4, 5, 6     # MASKIOU_TILE_*
# every symbol include/maskiou.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("maskiou_version", "maskiou_last_error", "maskiou_tile", "maskiou_workspace_bytes",
                    "maskiou_pairwise", "maskiou_binarize")

_vp, _ci, _cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


class Shape(ctypes.Structure):
    """include/maskiou.h ``maskiou_shape``."""
    _fields_ = [(name, _ci) for name in ("Na", "Nb", "F", "h", "w", "H", "W")]


def _prototypes(lib):
    shape_p = ctypes.POINTER(Shape)
    lib.maskiou_tile.restype = _ci
    lib.maskiou_tile.argtypes = [_ci]
    lib.maskiou_workspace_bytes.restype = ctypes.c_longlong
    lib.maskiou_workspace_bytes.argtypes = [_ci, shape_p]
    lib.maskiou_pairwise.restype = _ci
    lib.maskiou_pairwise.argtypes = [_ci, _ci, _vp, _vp, shape_p, _cd, _vp, _vp, _vp, _vp, _vp, _vp]
    lib.maskiou_binarize.restype = _ci
    lib.maskiou_binarize.argtypes = [_ci, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _vp, _vp]


# load(): the library with the maskiou_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("maskiou", MASKIOU_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


def tile(which):
    """A constant of the kernels' tiling (maskiou_tile): the pairwise pass owns ``TILE_BLOCK`` x ``TILE_BLOCK`` entries per
    workgroup and walks pixel tiles of ``TILE_ROWS`` x ``TILE_COLS``; a frame's tiles are cut into at most
    ``TILE_MAX_SPLITS`` split ranges of at least ``TILE_SPLIT_TILES`` tiles; binarise writes ``TILE_BIN_PIXELS`` bytes per
    workgroup and keeps ``TILE_BIN_SRC`` source elements in LDS."""
    return _check(load().maskiou_tile(which), "maskiou_tile")


def splits(H, W):
    """(tiles per frame, tiles per split range, split ranges per frame) of a target size: the rule of include/maskiou.h,
    restated for the tests and the documentation."""
    tiles = -(-H // tile(TILE_ROWS)) * -(-W // tile(TILE_COLS))
    per = max(tile(TILE_SPLIT_TILES), -(-tiles // tile(TILE_MAX_SPLITS)))
    return tiles, per, -(-tiles // per)


def workspace_bytes(code, shape):
    """Bytes of the workspace of :func:`pairwise` (maskiou_workspace_bytes)."""
    return _check(load().maskiou_workspace_bytes(code, ctypes.byref(shape)), "maskiou_workspace_bytes")


def pairwise(code, reduce, a, b, shape, eps, workspace, inter, sum_a, sum_b, iou):
    """maskiou_pairwise on the current stream: ``inter`` [F, Na, Nb], ``sum_a`` [F, Na], ``sum_b`` [F, Nb] and ``iou``
    [Na, Nb], fully written."""
    with _native._on(a.device):
        rc = load().maskiou_pairwise(code, reduce, _native._p(a), _native._p(b), ctypes.byref(shape), float(eps),
                                     _native._p(workspace), _native._p(inter), _native._p(sum_a), _native._p(sum_b),
                                     _native._p(iou), _native._stream(a))
    _check(rc, "maskiou_pairwise")


def binarize(code, layout, src, N, h, w, H, W, out):
    """maskiou_binarize on the current stream: ``out`` [N, H, W] or [N, W, H] bytes, fully written."""
    with _native._on(src.device):
        rc = load().maskiou_binarize(code, layout, _native._p(src), N, h, w, H, W, _native._p(out), _native._stream(src))
    _check(rc, "maskiou_binarize")
