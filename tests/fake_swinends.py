"""Test double for devis_amd._swinends (tests/ only): the CONTRACT of the swinends_* entry points (include/swinends.h) on CPU
tensors, by tests/swinends_oracle.py, so the host logic -- the two autograd Functions, which gradients are computed, the patched
``PatchEmbed`` and ``SwinTransformer`` -- can be tested without a GPU.  It takes float64 as well.  The product never imports
this."""
import torch

import swinends_oracle as O


def install(monkeypatch, calls=None):
    """Patch devis_amd so that CPU tensors (float64 included) are accepted and computed here; ``calls`` (a list) records
    ("embed_forward", has norm, has bias, statistics asked), ("embed_backward", grad_proj_weight, grad_proj_bias, grad_norm_weight,
    grad_norm_bias), ("map_forward", H, W, C) and ("map_backward", grad_x, grad_weight, grad_bias)."""
    from devis_amd import _swinends
    from devis_amd.functions import swin_ends
    from devis_amd.modules import swin_ends as module
    calls = [] if calls is None else calls

    def put(dst, src):
        if dst is not None:
            dst.copy_(src.reshape(dst.shape))

    def embed_forward(types, image, proj_weight, proj_bias, norm_weight, norm_bias, eps, shape, tokens, mean, rstd):
        calls.append(("embed_forward", norm_weight is not None, proj_bias is not None, mean is not None))
        assert image.is_contiguous() and proj_weight.is_contiguous() and (mean is None) == (rstd is None)
        assert tuple(image.shape) == (shape.B, shape.Cin, shape.H, shape.W) and tuple(proj_weight.shape) == (shape.C, shape.Cin, shape.p, shape.p)
        got = O.embed_forward(image, proj_weight, proj_bias, norm_weight, norm_bias, eps)
        put(tokens, got["tokens"])
        if mean is not None:
            assert mean.dtype == torch.float32
            put(mean, got["mean"])
            put(rstd, got["rstd"])

    def embed_backward(types, image, proj_weight, proj_bias, norm_weight, mean, rstd, grad_tokens, shape, workspace, grad_proj_weight,
                       grad_proj_bias, grad_norm_weight, grad_norm_bias):
        outs = (grad_proj_weight, grad_proj_bias, grad_norm_weight, grad_norm_bias)
        calls.append(("embed_backward",) + tuple(t is not None for t in outs))
        assert grad_tokens.is_contiguous() and workspace is not None and (norm_weight is None) == (mean is None)
        got = O.embed_grads(image, proj_weight, proj_bias, norm_weight, None, grad_tokens, stats=None if mean is None else (mean, rstd))
        for dst, name in zip(outs, ("grad_proj_weight", "grad_proj_bias", "grad_norm_weight", "grad_norm_bias")):
            put(dst, got[name]) if dst is not None else None

    def map_forward(types, x, weight, bias, eps, shape, y, mean, rstd):
        calls.append(("map_forward", shape.H, shape.W, shape.C))
        assert x.is_contiguous() and tuple(y.shape) == (shape.B, shape.C, shape.H, shape.W) and y.is_contiguous()
        got = O.map_forward(x, shape.H, shape.W, weight, bias, eps)
        put(y, got["y"])
        put(mean, got["mean"])
        put(rstd, got["rstd"])

    def map_backward(types, x, weight, mean, rstd, grad_y, shape, workspace, grad_x, grad_weight, grad_bias):
        calls.append(("map_backward", grad_x is not None, grad_weight is not None, grad_bias is not None))
        assert grad_y.is_contiguous() and tuple(grad_y.shape) == (shape.B, shape.C, shape.H, shape.W)
        assert (workspace is not None) == (grad_weight is not None or grad_bias is not None)
        got = O.map_grads(x, shape.H, shape.W, weight, None, grad_y, stats=(mean, rstd))
        put(grad_x, got["grad_x"])
        put(grad_weight, got["grad_weight"])
        put(grad_bias, got["grad_bias"])

    monkeypatch.setattr(swin_ends, "_check_device", lambda *a: None)
    monkeypatch.setattr(swin_ends, "_on_gpu", lambda t: True)
    monkeypatch.setattr(module, "_on_gpu", lambda t: True)
    monkeypatch.setattr(swin_ends, "DTYPES", swin_ends.DTYPES + (torch.float64,))
    monkeypatch.setattr(_swinends, "embed_types_of", lambda *dtypes: dtypes)
    monkeypatch.setattr(_swinends, "map_types_of", lambda *dtypes: dtypes)
    monkeypatch.setattr(_swinends, "embed_workspace_bytes", lambda shape, want: 256)
    monkeypatch.setattr(_swinends, "map_workspace_bytes", lambda shape: 256)
    for f in (embed_forward, embed_backward, map_forward, map_backward):
        monkeypatch.setattr(_swinends, f.__name__, f)
    return calls
