"""Test double for devis_amd._winattn (tests/ only): the CONTRACT of the winattn_* entry points (include/winattn.h) on CPU
tensors in plain torch, by the chain of tests/winattn_oracle.py, so the host logic -- the autograd Function, which gradients are
computed, the block's forward, the patch -- can be tested without a GPU.  It takes float64 as well, and computes in the
operands' dtype (float32 for 16-bit).  The product never imports this."""
import torch

import winattn_oracle as O


def _acc(t):
    return t.dtype if t.dtype in (torch.float32, torch.float64) else torch.float32


def _geometry(shape):
    return int(shape.heads), int(shape.window), int(shape.shift)


def install(monkeypatch, calls=None):
    """Patch devis_amd so that CPU tensors (float64 included) are accepted and computed here; ``calls`` (a list) records the
    entry points' names, for backward together with which outputs were asked for."""
    from devis_amd import _winattn
    from devis_amd.functions import window_attention
    from devis_amd.modules import window_attention as module
    calls = [] if calls is None else calls

    def check(qkv, table, shape, wide):
        assert qkv.is_contiguous() and table.is_contiguous()
        assert tuple(qkv.shape) == (shape.B, shape.Hp, shape.Wp, 3 * shape.heads * shape.head_dim)
        assert tuple(table.shape) == ((2 * shape.window - 1) ** 2, shape.heads)
        assert bool(wide) == (table.dtype != qkv.dtype)

    def forward(code, wide, qkv, table, scale, shape, out, lse, out_acc=None):
        calls.append("forward")
        check(qkv, table, shape, wide)
        H, ws, shift = _geometry(shape)
        acc = _acc(qkv)
        result = O.attention(qkv.to(acc), table.to(acc), H, ws, shift, scale)
        out.copy_(result)
        if out_acc is not None:              # before the rounding to a 16-bit dtype
            out_acc.copy_(result)
        if lse is not None:
            assert tuple(lse.shape) == (shape.B, (shape.Hp // ws) * (shape.Wp // ws), H, ws * ws) and lse.dtype == torch.float32
            lse.zero_()                      # (the double's backward recomputes everything)
        return 1

    def backward(code, wide, qkv, table, out, grad_out, lse, scale, shape, grad_qkv, grad_table, workspace):
        calls.append(("backward", grad_qkv is not None, grad_table is not None))
        check(qkv, table, shape, wide)
        assert out.dtype == _acc(qkv), "the backward takes out in the arithmetic type: the forward's out_acc for 16-bit operands"
        assert (workspace is not None) == (grad_table is not None)
        H, ws, shift = _geometry(shape)
        acc = _acc(qkv)
        with torch.enable_grad():
            a, b = qkv.detach().to(acc).requires_grad_(True), table.detach().to(acc).requires_grad_(True)
            result = O.attention(a, b, H, ws, shift, scale)
            wanted = [t for t, g in ((a, grad_qkv), (b, grad_table)) if g is not None]
            grads = list(torch.autograd.grad(result, wanted, grad_out.to(acc)))
        if grad_qkv is not None:
            grad_qkv.copy_(grads.pop(0))
        if grad_table is not None:
            grad_table.copy_(grads.pop(0))
        return 2 * (grad_qkv is not None) + 3 * (grad_table is not None)

    monkeypatch.setattr(window_attention, "_check_device", lambda *a: None)
    monkeypatch.setattr(window_attention, "DTYPES", window_attention.DTYPES + (torch.float64,))
    monkeypatch.setattr(module, "_on_gpu", lambda x: True)
    monkeypatch.setattr(_winattn, "forward", forward)
    monkeypatch.setattr(_winattn, "backward", backward)
    monkeypatch.setattr(_winattn, "workspace_bytes", lambda shape: 16)
    return calls
