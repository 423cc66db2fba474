"""Test double for devis_amd._prenorm (tests/ only): the CONTRACT of the prenorm_* entry points (include/prenorm.h) on CPU
tensors, by tests/prenorm_oracle.py, so the host logic -- the two autograd Functions, which gradients are computed, the patched
blocks, layers and patch merging -- can be tested without a GPU.  It takes float64 as well.  The product never imports this."""
import torch

import prenorm_oracle as O

PLAIN, RESIDUAL, MERGE = 0, 1, 2


def _forms(shape, x):
    """(x as [B, L, C], merge, map_size) of a prenorm_shape."""
    B, H, W = int(shape.B), int(shape.H), int(shape.W)
    merge = (H, W) if shape.source == MERGE else None
    map_size = (H, W, int(shape.Hp), int(shape.Wp)) if shape.dest == 1 else None
    C = shape.C // 4 if merge else shape.C
    return x.reshape(B, H * W, C), merge, map_size


def install(monkeypatch, calls=None):
    """Patch devis_amd so that CPU tensors (float64 included) are accepted and computed here; ``calls`` (a list) records
    ("forward", source, dest, has keep) and ("backward", source, dest, grad_x, grad_delta, grad_weight, grad_bias, grad_s
    given)."""
    from devis_amd import _prenorm
    from devis_amd.functions import pre_norm
    calls = [] if calls is None else calls

    def forward(types, x, delta, keep, weight, bias, eps, shape, s, y, mean, rstd):
        calls.append(("forward", int(shape.source), int(shape.dest), keep is not None))
        assert x.is_contiguous() and (delta is None) == (shape.source != RESIDUAL) and (s is None) == (delta is None)
        assert keep is None or (keep.dtype == torch.float32 and tuple(keep.shape) == (shape.B,))
        xs, merge, map_size = _forms(shape, x)
        got = O.forward(xs, None if delta is None else delta.reshape(xs.shape), weight, bias, eps, keep, merge, map_size,
                        None if x.dtype == torch.float64 else x.dtype)
        y.copy_(got["y"].view(y.shape))
        if s is not None:
            s.copy_(got["s"].view(s.shape))
        if mean is not None:
            assert mean.dtype == torch.float32 and mean.numel() == got["mean"].numel()
            mean.copy_(got["mean"].view(mean.shape))
            rstd.copy_(got["rstd"].view(rstd.shape))

    def backward(types, x, keep, weight, mean, rstd, grad_y, grad_s, shape, workspace, grad_x, grad_delta, grad_weight, grad_bias):
        calls.append(("backward", int(shape.source), int(shape.dest), grad_x is not None, grad_delta is not None,
                      grad_weight is not None, grad_bias is not None, grad_s is not None))
        assert x.is_contiguous() and grad_y.is_contiguous()
        xs, merge, map_size = _forms(shape, x)
        # (x is the forward's s in the residual form: the oracle's PLAIN form on it gives dz)
        got = O.grads(xs, None, weight, None, None, grad_y, grad_s, None, merge, map_size, stats=(mean, rstd))
        if grad_x is not None:
            grad_x.copy_(got["grad_x"].view(grad_x.shape))
        if grad_delta is not None:
            k = torch.ones(shape.B, dtype=torch.float64) if keep is None else keep.double()
            grad_delta.copy_((got["grad_x"] * k.view(-1, 1, 1)).view(grad_delta.shape))
        if grad_weight is not None:
            grad_weight.copy_(got["grad_weight"])
        if grad_bias is not None:
            grad_bias.copy_(got["grad_bias"])

    monkeypatch.setattr(pre_norm, "_check_device", lambda *a: None)
    monkeypatch.setattr(pre_norm, "_on_gpu", lambda t: True)
    monkeypatch.setattr(pre_norm, "DTYPES", pre_norm.DTYPES + (torch.float64,))
    monkeypatch.setattr(_prenorm, "types_of", lambda *dtypes: dtypes)
    monkeypatch.setattr(_prenorm, "workspace_bytes", lambda shape: 0)
    monkeypatch.setattr(_prenorm, "forward", forward)
    monkeypatch.setattr(_prenorm, "backward", backward)
    return calls
