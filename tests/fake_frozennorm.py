"""Test double for devis_amd._frozennorm (tests/ only): the CONTRACT of the frozennorm_* entry points (include/frozennorm.h) on
CPU tensors, by tests/frozennorm_oracle.py, so the host logic -- the autograd Function, which gradients are computed, the patched
blocks and stem -- can be tested without a GPU.  It takes float64 as well.  The product never imports this."""
import torch

import frozennorm_oracle as O

NCHW, NHWC = 0, 1


def _in_layout(t, layout):
    return t.is_contiguous() if layout == NCHW else t.is_contiguous(memory_format=torch.channels_last)


def _checked(shape, *tensors):
    dims = (int(shape.N), int(shape.C), int(shape.H), int(shape.W))
    for t in tensors:
        assert t is None or (tuple(t.shape) == dims and _in_layout(t, int(shape.layout))), (dims, t.shape, t.stride())


def _norm_ok(norm, full=True):
    assert len(norm) == 5 and isinstance(norm[4], float)
    for t in norm[:4] if full else (norm[0], norm[3]):
        assert t.is_contiguous() and not t.requires_grad


def install(monkeypatch, calls=None):
    """Patch devis_amd so that CPU tensors (float64 included) are accepted and computed here; ``calls`` (a list) records
    ("forward", residual form, relu, layout), ("backward", residual form, relu, grad_x given, grad_r given) and
    ("pool", layout)."""
    from devis_amd import _frozennorm
    from devis_amd.functions import frozen_norm
    calls = [] if calls is None else calls

    def forward(types, shape, x, norm, r, norm_r, y):
        form = int(shape.residual)
        calls.append(("forward", form, int(shape.relu), int(shape.layout)))
        _checked(shape, x, r, y)
        assert (r is None) == (form == O.NONE) and (norm_r is None) == (form != O.NORMED)
        assert types == (x.dtype, x.dtype if r is None else r.dtype, y.dtype)
        _norm_ok(norm)
        if norm_r is not None:
            _norm_ok(norm_r)
        y.copy_(O.forward(x, norm, r, norm_r, bool(shape.relu))[0])

    def backward(types, shape, grad_y, y, norm, norm_r, grad_x, grad_r):
        form = int(shape.residual)
        calls.append(("backward", form, int(shape.relu), grad_x is not None, grad_r is not None))
        _checked(shape, grad_y, y, grad_x, grad_r)
        assert grad_x is not None or grad_r is not None
        assert (y is None) == (not shape.relu) and (grad_r is None or form != O.NONE)
        assert (norm is None) == (grad_x is None) and (norm_r is None) == (grad_r is None or form != O.NORMED)
        C = int(shape.C)
        unit = (torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C), 0.0)       # (stands in for a norm that is not read)
        gx, gr = O.backward(grad_y, y, norm or unit, form, norm_r or unit, bool(shape.relu))
        if grad_x is not None:
            grad_x.copy_(gx[0])
        if grad_r is not None:
            grad_r.copy_(gr[0])

    def pool_forward(types, shape, x, norm, y):
        calls.append(("pool", int(shape.layout)))
        _checked(shape, x)
        assert int(shape.residual) == O.NONE and _in_layout(y, int(shape.layout))
        _norm_ok(norm)
        y.copy_(O.pool(x, norm)[0])

    monkeypatch.setattr(frozen_norm, "_check_device", lambda *a: None)
    monkeypatch.setattr(frozen_norm, "_on_gpu", lambda t: True)
    monkeypatch.setattr(frozen_norm, "DTYPES", frozen_norm.DTYPES + (torch.float64,))
    monkeypatch.setattr(frozen_norm, "BUFFER_DTYPES", frozen_norm.BUFFER_DTYPES + (torch.float64,))
    monkeypatch.setattr(_frozennorm, "types_of", lambda *dtypes: dtypes)
    monkeypatch.setattr(_frozennorm, "forward", forward)
    monkeypatch.setattr(_frozennorm, "backward", backward)
    monkeypatch.setattr(_frozennorm, "pool_forward", pool_forward)
    return calls
