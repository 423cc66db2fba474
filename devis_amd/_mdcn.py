"""ctypes binding of include/mdcn.h: the deformable-convolution entry points of libmsda_hip.so (the library ``_native.load()``
opens).  As in ``_native``: no fallback, a failing call raises, launches go to the current stream, and the library neither
allocates nor synchronises -- the column buffers are torch tensors of the caller.
"""
import ctypes

import torch

from . import _binding, _native

MDCN_ABI_VERSION = 2
GRAD_INPUT, GRAD_SAMPLING = 1, 2        # include/mdcn.h MDCN_GRAD_INPUT / MDCN_GRAD_SAMPLING
# every symbol include/mdcn.h declares (tests check the library exports each of them)
EXPORTED_SYMBOLS = ("mdcn_version", "mdcn_last_error", "mdcn_workspace_bytes", "mdcn_im2col", "mdcn_backward",
                    "mdcn_fixed_workspace_bytes", "mdcn_backward_input_fixed")
_OFF32_CODE = {torch.bfloat16: 4, torch.float16: 5}     # MDCN_BF16_OFF32 / MDCN_F16_OFF32

_vp, _ci = ctypes.c_void_p, ctypes.c_int


class Shape(ctypes.Structure):
    """include/mdcn.h ``mdcn_shape``."""
    _fields_ = [(name, _ci) for name in ("N", "C", "H", "W", "Ho", "Wo", "Kh", "Kw", "stride_h", "stride_w", "pad_h", "pad_w",
                                         "dil_h", "dil_w", "G")]


def _prototypes(lib):
    shape_p = ctypes.POINTER(Shape)
    lib.mdcn_workspace_bytes.restype = ctypes.c_longlong
    lib.mdcn_workspace_bytes.argtypes = [_ci, shape_p, _ci]
    lib.mdcn_im2col.restype = _ci
    lib.mdcn_im2col.argtypes = [_ci, _vp, _vp, _vp, shape_p, _vp, _vp]
    lib.mdcn_backward.restype = _ci
    lib.mdcn_backward.argtypes = [_ci, _ci, _vp, _vp, _vp, _vp, shape_p, _vp, _vp, _vp, _vp]
    lib.mdcn_fixed_workspace_bytes.restype = ctypes.c_longlong
    lib.mdcn_fixed_workspace_bytes.argtypes = [_ci, shape_p, _ci]
    lib.mdcn_backward_input_fixed.restype = _ci
    lib.mdcn_backward_input_fixed.argtypes = [_ci, _vp, _vp, _vp, shape_p, _vp, _vp, _vp]


# load(): the library with the mdcn_* prototypes set; raises RuntimeError when it cannot be loaded or is another version
load, _check = _binding.bind("mdcn", MDCN_ABI_VERSION, EXPORTED_SYMBOLS, _prototypes)


def type_code(dtype, offset_dtype):
    """mdcn_dtype of a call whose input / columns are ``dtype`` and whose offset / mask are ``offset_dtype``: the same type,
    or float32 beside a 16-bit input."""
    if offset_dtype == dtype:
        return _native.dtype_code(dtype)
    if offset_dtype == torch.float32 and dtype in _OFF32_CODE:
        return _OFF32_CODE[dtype]
    raise RuntimeError("devis_amd: offset / mask must have input's dtype (or float32 beside a 16-bit input), got %s beside %s"
                       % (offset_dtype, dtype))


def workspace_bytes(code, shape, batch):
    """Bytes of the column buffer of ``batch`` images (mdcn_workspace_bytes)."""
    return _check(load().mdcn_workspace_bytes(code, ctypes.byref(shape), batch), "mdcn_workspace_bytes")


def im2col(code, x_nhwc, offset, mask, shape, columns):
    """mdcn_im2col on the current stream: ``x_nhwc`` [N, H, W, C], ``offset`` / ``mask`` (or None) NCHW -> ``columns``."""
    with _native._on(x_nhwc.device):
        rc = load().mdcn_im2col(code, _native._p(x_nhwc), _native._p(offset), _native._p(mask), ctypes.byref(shape),
                                _native._p(columns), _native._stream(x_nhwc))
    _check(rc, "mdcn_im2col")


def backward(grads, code, x_nhwc, offset, mask, grad_columns, shape, grad_input_acc, grad_offset, grad_mask):
    """mdcn_backward on the current stream for the gradient groups in ``grads``; outputs of a group that is not asked for
    may be None.  ``grad_input_acc`` ([N, H, W, C] in the arithmetic type) is accumulated into."""
    with _native._on(x_nhwc.device):
        rc = load().mdcn_backward(grads, code, _native._p(x_nhwc), _native._p(offset), _native._p(mask),
                                  _native._p(grad_columns), ctypes.byref(shape), _native._p(grad_input_acc),
                                  _native._p(grad_offset), _native._p(grad_mask), _native._stream(x_nhwc))
    _check(rc, "mdcn_backward")


def fixed_workspace_bytes(code, shape, batch):
    """Bytes of the workspace of :func:`backward_input_fixed` for ``batch`` images (mdcn_fixed_workspace_bytes)."""
    return _check(load().mdcn_fixed_workspace_bytes(code, ctypes.byref(shape), batch), "mdcn_fixed_workspace_bytes")


def backward_input_fixed(code, offset, mask, grad_columns, shape, workspace, grad_input):
    """mdcn_backward_input_fixed on the current stream: the order-independent grad_input of ``shape.N`` images, fully
    written into ``grad_input`` ([N, H, W, C] in the arithmetic type).  ``workspace`` is a tensor of at least
    :func:`fixed_workspace_bytes` bytes; it need not be initialised."""
    with _native._on(grad_columns.device):
        rc = load().mdcn_backward_input_fixed(code, _native._p(offset), _native._p(mask), _native._p(grad_columns),
                                              ctypes.byref(shape), _native._p(workspace), _native._p(grad_input),
                                              _native._stream(grad_columns))
    _check(rc, "mdcn_backward_input_fixed")
