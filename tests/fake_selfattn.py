"""Test double for devis_amd._selfattn (tests/ only): the CONTRACT of the selfattn_* entry points (include/selfattn.h) on CPU
tensors in plain torch, with the mask of tests/selfattn_oracle.py, so the host logic -- the autograd Function, which gradients
are computed, the drop-in module, the patch -- can be tested without a GPU.  It takes float64 as well, and computes in the
operands' dtype (float32 for 16-bit).  The product never imports this."""
import math

import torch

import selfattn_oracle as O


def _acc(t):
    return t.dtype if t.dtype in (torch.float32, torch.float64) else torch.float32


def _parts(q, k, v, seed, p, shape):
    """(q, k, v as [N, H, rows, D] in the arithmetic type, dropout(P) and P [N, H, L, S], 1 / sqrt(D))."""
    L, S, N, E, H = shape.L, shape.S, shape.N, shape.E, shape.H
    D = E // H
    acc = _acc(q)
    heads = lambda t, rows: t.to(acc).reshape(rows, N, H, D).permute(1, 2, 0, 3)      # noqa: E731
    qh, kh, vh = heads(q, L), heads(k, S), heads(v, S)
    prob = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(D), -1)
    dropped = prob * O.scale_of(p)
    keep = None
    if seed is not None and p > 0.0:
        keep = O.keep_mask(int(seed.item()), N, H, L, S, p)
        dropped = torch.where(keep, dropped, torch.zeros_like(dropped))
    return qh, kh, vh, prob, dropped, keep, 1.0 / math.sqrt(D)


def install(monkeypatch, calls=None):
    """Patch devis_amd so that CPU tensors (float64 included) are accepted and computed here; ``calls`` (a list) records the
    entry points' names, for backward together with which outputs were asked for."""
    from devis_amd import _selfattn
    from devis_amd.functions import self_attention
    from devis_amd.modules import self_attention as module
    calls = [] if calls is None else calls

    def merge(t, like):          # [N, H, rows, D] -> like's [rows, N, E]
        return t.permute(2, 0, 1, 3).reshape(like.shape)

    def forward(code, q, k, v, seed, p, shape, out, lse, out_acc=None):
        calls.append("forward")
        qh, kh, vh, prob, dropped, keep, inv = _parts(q, k, v, seed, p, shape)
        out.copy_(merge(dropped @ vh, out))
        if out_acc is not None:              # before the rounding to a 16-bit dtype
            out_acc.copy_(merge(dropped @ vh, out_acc))
        if lse is not None:
            lse.copy_(torch.logsumexp(qh @ kh.transpose(-1, -2) * inv, -1).reshape(lse.shape))
        return 1

    def backward(code, q, k, v, out, grad_out, lse, seed, p, shape, grad_q, grad_k, grad_v):
        calls.append(("backward", grad_q is not None, grad_k is not None, grad_v is not None))
        assert out.dtype == _acc(q), "the backward takes out in the arithmetic type: the forward's out_acc for 16-bit operands"
        qh, kh, vh, prob, dropped, keep, inv = _parts(q, k, v, seed, p, shape)
        L, N, H = shape.L, shape.N, shape.H
        do = grad_out.to(qh.dtype).reshape(L, N, H, -1).permute(1, 2, 0, 3)
        o = out.to(qh.dtype).reshape(L, N, H, -1).permute(1, 2, 0, 3)
        dp = (do @ vh.transpose(-1, -2)) * O.scale_of(p)
        if keep is not None:
            dp = torch.where(keep, dp, torch.zeros_like(dp))
        ds = prob * (dp - (do * o).sum(-1, keepdim=True))
        if grad_q is not None:
            grad_q.copy_(merge(ds @ kh * inv, grad_q))
        if grad_k is not None:
            grad_k.copy_(merge(ds.transpose(-1, -2) @ qh * inv, grad_k))
        if grad_v is not None:
            grad_v.copy_(merge(dropped.transpose(-1, -2) @ do, grad_v))
        return (grad_q is not None) + (grad_k is not None or grad_v is not None)

    monkeypatch.setattr(self_attention, "_check_device", lambda *a: None)
    monkeypatch.setattr(self_attention, "DTYPES", self_attention.DTYPES + (torch.float64,))
    monkeypatch.setattr(module, "_on_gpu", lambda x: True)
    monkeypatch.setattr(_selfattn, "forward", forward)
    monkeypatch.setattr(_selfattn, "backward", backward)
    return calls
