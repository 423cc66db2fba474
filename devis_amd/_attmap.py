"""ctypes binding of include/attmap.h: the attention-map entry points of libmsda_hip.so (the library ``_native.load()``
opens).  As in ``_mdcn``: no fallback, a failing call raises, launches go to the current stream, and the library neither
allocates nor synchronises -- outputs and workspaces are torch tensors of the caller.
"""
import ctypes

import torch

from . import _binding, _native

ATTMAP_ABI_VERSION = 1
GRAD_Q, GRAD_K = 1, 2       # include/attmap.h ATTMAP_GRAD_Q / ATTMAP_GRAD_K
# every symbol include/attmap.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("attmap_version", "attmap_last_error", "attmap_workspace_bytes", "attmap_forward", "attmap_backward")

_vp, _ci = ctypes.c_void_p, ctypes.c_int


class Shape(ctypes.Structure):
    """include/attmap.h ``attmap_shape``."""
    _fields_ = [(name, _ci) for name in ("B", "Q", "n", "c", "H", "W")]


def _prototypes(lib):
    shape_p = ctypes.POINTER(Shape)
    lib.attmap_workspace_bytes.restype = ctypes.c_longlong
    lib.attmap_workspace_bytes.argtypes = [_ci, shape_p]
    lib.attmap_forward.restype = _ci
    lib.attmap_forward.argtypes = [_ci, _ci, _vp, _vp, _vp, shape_p, ctypes.c_double, _vp, _vp, _vp]
    lib.attmap_backward.restype = _ci
    lib.attmap_backward.argtypes = [_ci, _ci, _ci, _vp, _vp, shape_p, ctypes.c_double, _vp, _vp, _vp]


# load(): the library with the attmap_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("attmap", ATTMAP_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


def out_dtype(dtype, requested):
    """The storage type of ``out`` beside ``dtype`` inputs: ``dtype`` itself (also for None), or float32 beside 16-bit
    inputs -- nothing else."""
    if requested is None or requested == dtype:
        return dtype
    if requested == torch.float32 and dtype in (torch.bfloat16, torch.float16):
        return requested
    raise RuntimeError("devis_amd: attention_maps: out_dtype must be the inputs' dtype (or float32 beside 16-bit inputs), got "
                       "%s beside %s" % (requested, dtype))


def workspace_bytes(code, shape):
    """Bytes of the workspace of :func:`forward` and :func:`backward` (attmap_workspace_bytes)."""
    return _check(load().attmap_workspace_bytes(code, ctypes.byref(shape)), "attmap_workspace_bytes")


def forward(code, out_code, q, k, mask, shape, scale, workspace, out):
    """attmap_forward on the current stream: ``q`` [B, Q, n*c], ``k`` [B, n*c, H, W], ``mask`` [B, H, W] bytes or None ->
    ``out`` [B, Q, n, H, W], fully written."""
    with _native._on(q.device):
        rc = load().attmap_forward(code, out_code, _native._p(q), _native._p(k), _native._p(mask), ctypes.byref(shape),
                                   float(scale), _native._p(workspace), _native._p(out), _native._stream(q))
    _check(rc, "attmap_forward")


def backward(grads, code, out_code, out, grad_out, shape, scale, workspace, dl):
    """attmap_backward on the current stream: ``dl`` [B, n, Q, H*W] = scale * out * (grad_out - rowsum(grad_out * out)),
    fully written."""
    with _native._on(out.device):
        rc = load().attmap_backward(grads, code, out_code, _native._p(out), _native._p(grad_out), ctypes.byref(shape),
                                    float(scale), _native._p(workspace), _native._p(dl), _native._stream(out))
    _check(rc, "attmap_backward")
