"""Test double for devis_amd._addnorm (tests/ only): the CONTRACT of the addnorm_* entry points (include/addnorm.h) on CPU
tensors in plain torch, with the mask of tests/addnorm_oracle.py, so the host logic -- the two autograd Functions, which
gradients are computed, the patched layers -- can be tested without a GPU.  The product never imports this."""
import torch

import addnorm_oracle as O


def _acc(t):
    return torch.float64 if t.dtype == torch.float64 else torch.float32


def _keep(seed, R, C, p):
    return None if seed is None or p == 0.0 else O.keep_mask(int(seed.item()), R, C, p)


def _z(x, delta, seed, p, R, C):
    acc = _acc(x)
    keep = _keep(seed, R, C, p)
    d = delta.reshape(R, C).to(acc) * O.scale_of(p)
    if keep is not None:
        d = torch.where(keep, d, torch.zeros_like(d))
    return x.reshape(R, C).to(acc) + d, keep


def install(monkeypatch, calls=None):
    """Patch devis_amd so that CPU tensors are accepted and computed here; ``calls`` (a list) records the entry points'
    names, for backward together with which outputs were asked for."""
    from devis_amd import _addnorm
    from devis_amd.functions import add_norm
    calls = [] if calls is None else calls

    def forward(types, x, delta, weight, bias, seed, p, eps, shape, y, mean, rstd):
        calls.append("forward")
        R, C = shape.R, shape.C
        z, _ = _z(x, delta, seed, p, R, C)
        m = z.mean(1, keepdim=True)
        rs = 1 / torch.sqrt(((z - m) ** 2).mean(1, keepdim=True) + eps)
        y.copy_((((z - m) * rs) * weight.to(z.dtype) + bias.to(z.dtype)).view(y.shape))
        if mean is not None:
            mean.copy_(m.view(mean.shape))
            rstd.copy_(rs.view(rstd.shape))

    def backward(types, x, delta, weight, seed, p, mean, rstd, grad_y, shape, workspace, grad_x, grad_delta, grad_weight, grad_bias):
        calls.append(("backward", grad_x is not None, grad_delta is not None, grad_weight is not None, grad_bias is not None))
        R, C = shape.R, shape.C
        z, keep = _z(x, delta, seed, p, R, C)
        m, rs, g = mean.reshape(R, 1), rstd.reshape(R, 1), grad_y.reshape(R, C).to(z.dtype)
        xhat = (z - m) * rs
        gw = g * weight.to(z.dtype)
        dz = ((gw - gw.mean(1, keepdim=True)) - xhat * (gw * xhat).mean(1, keepdim=True)) * rs
        if grad_x is not None:
            grad_x.copy_(dz.view(grad_x.shape))
        if grad_delta is not None:
            dd = dz * O.scale_of(p)
            grad_delta.copy_((dd if keep is None else torch.where(keep, dd, torch.zeros_like(dd))).view(grad_delta.shape))
        if grad_weight is not None:
            grad_weight.copy_((g * xhat).sum(0))
        if grad_bias is not None:
            grad_bias.copy_(g.sum(0))

    def relu_forward(code, x, seed, p, shape, y):
        calls.append("relu_forward")
        keep = _keep(seed, shape.R, shape.C, p)
        v = torch.where(x > 0, x.to(_acc(x)) * O.scale_of(p), torch.where(x != x, x, torch.zeros_like(x)).to(_acc(x)))
        if keep is not None:
            v = torch.where(keep.view(x.shape), v, torch.zeros_like(v))
        y.copy_(v)

    def relu_backward(code, y, grad_y, p, n, grad_x):
        calls.append("relu_backward")
        grad_x.copy_(torch.where(y > 0, grad_y.to(_acc(y)) * O.scale_of(p), torch.zeros_like(grad_y, dtype=_acc(y))))

    monkeypatch.setattr(add_norm, "_check_device", lambda *a: None)
    monkeypatch.setattr(_addnorm, "workspace_bytes", lambda code, shape: 0)
    for name, fn in (("forward", forward), ("backward", backward), ("relu_forward", relu_forward), ("relu_backward", relu_backward)):
        monkeypatch.setattr(_addnorm, name, fn)
    return calls
