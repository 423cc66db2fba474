"""CPU tests of the decoder's query self-attention: the oracle (against torch's own multi-head attention, the mask rule), the C
ABI of include/selfattn.h (exports, version, argument errors -- no compute calls), the host code (checks, errors, which
gradients are computed), the drop-in module and the patch with the binding replaced by the torch stand-in of
tests/fake_selfattn.py, the patched decoder layer on the reference's fixtures, and the compiled path.  The kernels themselves
are tests/test_selfattn_gpu.py."""
import collections
import copy
import ctypes
import json
import math
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import addnorm_oracle
import fake_addnorm
import fake_selfattn
import layerglue_cases as LG
import selfattn_cases as C
import selfattn_oracle as O
from conftest import ROOT

F32, F64 = torch.float32, torch.float64


def rand(*shape, seed=0, dtype=F64):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


# ---- oracle ------------------------------------------------------------------------------------------------------------------

def test_oracle_equals_torchs_multi_head_attention_in_float64():
    L, S, N, E, H = 11, 11, 2, 32, 8
    q, k, v, go = (rand(n, N, E, seed=i).requires_grad_(True) for i, n in enumerate((L, S, S, L)))
    eye, zero = torch.eye(E, dtype=F64), torch.zeros(E, dtype=F64)
    want = F.multi_head_attention_forward(q, k, v, E, H, torch.cat([eye] * 3), torch.cat([zero] * 3), None, None, False, 0.0, eye,
                                          zero, need_weights=False)[0]
    want_grads = torch.autograd.grad(want, (q, k, v), go)
    got = O.attention_grads(q, k, v, H, go)
    for a, b in zip(got, (want,) + want_grads):
        assert float((a - b).detach().abs().max()) <= 1e-12


def test_keep_mask_follows_the_rule_of_the_header():
    seed, N, H, L, S = 0x123456789ABCDEF, 2, 3, 5, 7
    keep = O.keep_mask(seed, N, H, L, S, 0.5)
    assert keep.shape == (N, H, L, S) and keep.dtype == torch.bool
    for n, h, i, j in ((0, 0, 0, 0), (1, 2, 4, 6), (1, 0, 3, 5), (0, 1, 2, 3)):
        row = (n * H + h) * L + i
        words = O.philox4x32_10((row, 0, j >> 2, 1), (seed & 0xffffffff, seed >> 32))
        assert bool(keep[n, h, i, j]) == (int(words[j & 3]) >= 1 << 31)
    # known answers: the four words of (seed 7, row 9, quad 2) and the mask they give at p = 0.5
    words = [int(w) for w in O.philox4x32_10((9, 0, 2, 1), (7, 0))]
    assert words == KNOWN_WORDS
    assert O.keep_mask(7, 1, 2, 5, 12, 0.5)[0, 1, 4, 8:12].tolist() == [w >= 1 << 31 for w in KNOWN_WORDS]
    assert O.keep_mask(seed, N, H, L, S, 0.0).all() and not O.keep_mask(seed, N, H, L, S, 1.0).any()
    # the last counter word separates the stream from addnorm's under an equal seed
    assert not torch.equal(O.keep_mask(seed, 1, 1, 8, 64, 0.5)[0, 0], addnorm_oracle.keep_mask(seed, 8, 64, 0.5))
    assert O.philox4x32_10 is addnorm_oracle.philox4x32_10 and O.threshold_of is addnorm_oracle.threshold_of


KNOWN_WORDS = [0xb2f4aa32, 0xc71b4076, 0xae996415, 0x384f6c31]          # Philox4x32-10(counter (9, 0, 2, 1), key (7, 0))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_kept_share_is_within_the_binomial_bound(p):
    n = 2 * 8 * 37 * 53
    share = float(O.keep_mask(20260101, 2, 8, 37, 53, p).double().mean())
    assert abs(share - (1 - p)) <= 6 * math.sqrt(p * (1 - p) / n), share


# ---- library -----------------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_selfattn_h_declares_and_versions_agree():
    from devis_amd import _addnorm, _native, _selfattn, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "selfattn.h")).read()
    declared = set(re.findall(r"\b(selfattn_[a-z_0-9]+)\s*\(", header.split("#ifndef SELFATTN_H")[1]))
    assert declared == set(_selfattn.EXPORTED_SYMBOLS) and len(declared) == 4
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _selfattn.load()
    assert lib.selfattn_version() == _selfattn.SELFATTN_ABI_VERSION == 2 == int(re.search(r"#define SELFATTN_ABI_VERSION (\d+)", header).group(1))
    assert dict(re.findall(r"SELFATTN_(F32|F64|BF16|F16) = (\d)", header)) == {"F32": "0", "F64": "1", "BF16": "2", "F16": "3"}
    assert int(re.search(r"#define SELFATTN_MAX_HEAD_DIM (\d+)", header).group(1)) == _selfattn.MAX_HEAD_DIM == 64
    assert ctypes.sizeof(_selfattn.Shape) == 40 and ctypes.sizeof(_selfattn.View) == 24
    assert _native.load().msda_build_info().decode() == "abi=14 arch=gfx950"              # no other ABI moved
    assert _addnorm.load().addnorm_version() == 1
    assert os.path.join(build.include_dir(), "selfattn.h") in build._headers()
    assert any(s.endswith("selfattn.hip") for s in build.sources())
    assert "selfattn.h" in open(os.path.join(ROOT, "setup.py")).read() and "selfattn.h" in build.include_dir.__doc__
    for phrase in ("Philox4x32-10", "row >> 32", "j >> 2, 1)", "floor(p * 2^32)", "row = (n * H + h) * L + i", "(j & 3)"):
        assert phrase in header, phrase


def test_selfattn_argument_errors_without_gpu():
    from devis_amd import _selfattn
    lib = _selfattn.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.selfattn_last_error
    shape = lambda L=5, S=6, N=2, E=32, H=8: ctypes.byref(_selfattn.Shape(L, S, N, E, H))        # noqa: E731
    view = lambda seq=64, batch=32, channel=1: ctypes.byref(_selfattn.View(seq, batch, channel))   # noqa: E731
    fwd = lambda dt=0, q=p, qv=view(), k=p, kv=view(), v=p, vv=view(), seed=p, pr=0.1, s=shape(), out=p, lse=p, acc=None: lib.selfattn_forward(      # noqa: E731
        dt, q, qv, k, kv, v, vv, seed, pr, s, out, lse, acc, None)
    bwd = lambda dt=0, q=p, qv=view(), k=p, kv=view(), v=p, vv=view(), out=p, go=p, lse=p, seed=p, pr=0.1, s=shape(), gq=p, gk=p, gv=p: lib.selfattn_backward(      # noqa: E731
        dt, q, qv, k, kv, v, vv, out, go, lse, seed, pr, s, gq, gk, gv, None)
    for call in (fwd, bwd):
        assert call(dt=9) == -1 and b"dtype" in err()
        assert call(dt=1) == -1 and b"float64" in err()
        assert call(s=None) == -1 and b"null pointer" in err()
        assert call(s=shape(L=-1)) == -1 and b"negative" in err()
        for name in ("L", "S", "N"):
            assert call(s=shape(**{name: 1 << 31})) == -1 and b"31 bits" in err(), name
        assert call(s=shape(E=1 << 33, H=1 << 29)) == -1 and b"31 bits" in err()
        assert call(s=shape(E=30, H=8)) == -1 and b"not divisible" in err()
        assert call(s=shape(E=0)) == -1 and call(s=shape(H=0)) == -1 and b"positive" in err()
        for E, H in ((24, 4), (8, 4), (68 * 2, 2), (3, 1)):                  # D = 6, 2, 68, 3
            assert call(s=shape(E=E, H=H)) == -1 and b"head dimension" in err(), (E, H)
        for bad in (-0.1, 1.5, float("nan")):
            assert call(pr=bad) == -1 and b"[0, 1]" in err()
        assert call(seed=None) == -1 and b"seed is required" in err()
        assert call(seed=None, pr=0.0, q=None) == -1 and b"null pointer" in err()          # (p == 0: no seed is needed)
        for name in ("qv", "kv", "vv"):
            assert call(**{name: None}) == -1 and b"null pointer" in err(), name
            assert call(**{name: view(channel=2)}) == -1 and b"last stride" in err(), name
            assert call(**{name: view(seq=1 << 31)}) == -1 and b"31 bits" in err(), name
            assert call(**{name: view(batch=1 << 31)}) == -1 and b"31 bits" in err(), name
            assert call(**{name: view(seq=-1)}) == -1 and b"31 bits" in err(), name
        for name in ("q", "k", "v", "out"):
            assert call(**{name: None}) == -1 and b"null pointer" in err(), name
        assert call(s=shape(N=1 << 20)) == -1 and b"65535" in err()
    for name in ("go", "lse"):
        assert bwd(**{name: None}) == -1 and b"null pointer" in err(), name
    # nothing to compute: nothing is launched, nothing is dereferenced
    nothing = dict(q=None, qv=None, k=None, kv=None, v=None, vv=None, out=None, lse=None)
    for empty in (shape(L=0), shape(N=0), shape(S=0)):
        assert fwd(s=empty, **nothing) == 0
        assert bwd(s=empty, go=None, gq=None, gk=None, gv=None, **nothing) == 0
        assert bwd(s=empty, go=None, **nothing) == 0
    assert bwd(gq=None, gk=None, gv=None, go=None, **nothing) == 0                       # no gradient is asked for


def test_operator_raises_on_cpu_tensors_and_on_bad_arguments_before_any_launch(monkeypatch):
    import devis_amd
    from devis_amd import _selfattn
    from devis_amd.functions import self_attention as A
    from devis_amd.modules import self_attention as M

    def no_launch(*a, **k):
        raise AssertionError("a kernel call was made")

    monkeypatch.setattr(_selfattn, "forward", no_launch)
    monkeypatch.setattr(_selfattn, "backward", no_launch)
    q, k, seed = torch.zeros(3, 2, 32), torch.zeros(5, 2, 32), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.multihead_attention(q, k, k, 8)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.multihead_attention(q.clone().requires_grad_(True), k, k, 8, p=0.5, seed=seed)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        A._backward(q, q, k, k, q, torch.zeros(16, 3), None, 8, 0.0, (True, True, True))
    for name in ("multihead_attention", "FusedMultiheadAttention", "patch_self_attention", "unpatch_self_attention"):
        assert name in devis_amd.__all__ and hasattr(devis_amd, name)
    assert devis_amd.multihead_attention is A.multihead_attention
    assert devis_amd.FusedMultiheadAttention is devis_amd.modules.FusedMultiheadAttention is M.FusedMultiheadAttention
    assert devis_amd.patch_self_attention is devis_amd.argument_builders.patch_self_attention
    assert devis_amd.unpatch_self_attention is devis_amd.argument_builders.unpatch_self_attention
    assert "no CPU path" in A.__doc__ and "IGNORES ``seed``" in A.__doc__

    meta = lambda *s, dtype=F32: torch.zeros(*s, dtype=dtype, device="meta")      # noqa: E731
    bf, f16 = torch.bfloat16, torch.float16
    assert A.check_shapes(meta(3, 2, 32), meta(5, 2, 32), meta(5, 2, 32), 8) == (3, 5, 2, 32, 8, 4)
    assert A.check_shapes(meta(0, 2, 64, dtype=bf), meta(0, 2, 64, dtype=bf), meta(0, 2, 64, dtype=bf), 1) == (0, 0, 2, 64, 1, 64)
    for dtype, D, ok in ((F32, 4, True), (bf, 32, True), (f16, 64, True), (F32, 20, True), (F64, 32, False), (F32, 68, False),
                         (F32, 6, False), (F32, 0, False), (torch.int32, 4, False)):
        assert A.supported(dtype, D) is ok, (dtype, D)
    bad = [
        (ValueError, "between 0 and 1", lambda: devis_amd.multihead_attention(q, k, k, 8, p=1.5, seed=seed)),
        (ValueError, "between 0 and 1", lambda: devis_amd.multihead_attention(q, k, k, 8, p=float("nan"), seed=seed)),
        (ValueError, "needs a seed", lambda: devis_amd.multihead_attention(q, k, k, 8, p=0.1)),
        (RuntimeError, "int64 tensor of one element", lambda: devis_amd.multihead_attention(q, k, k, 8, p=0.5, seed=torch.zeros(1))),
        (RuntimeError, "int64 tensor of one element", lambda: devis_amd.multihead_attention(q, k, k, 8, p=0.5, seed=torch.zeros(2, dtype=torch.int64))),
        (RuntimeError, "are required", lambda: A.check_shapes(meta(3, 32), meta(5, 32), meta(5, 32), 8)),
        (RuntimeError, "k and v must be", lambda: A.check_shapes(meta(3, 2, 32), meta(5, 2, 32), meta(4, 2, 32), 8)),
        (RuntimeError, "k and v must be", lambda: A.check_shapes(meta(3, 2, 32), meta(5, 3, 32), meta(5, 3, 32), 8)),
        (RuntimeError, "not divisible", lambda: A.check_shapes(meta(3, 2, 30), meta(5, 2, 30), meta(5, 2, 30), 8)),
        (RuntimeError, "head dimension", lambda: A.check_shapes(meta(3, 2, 24), meta(5, 2, 24), meta(5, 2, 24), 4)),
        (RuntimeError, "head dimension", lambda: A.check_shapes(meta(3, 2, 136), meta(5, 2, 136), meta(5, 2, 136), 2)),
        (RuntimeError, "one dtype", lambda: A.check_shapes(meta(3, 2, 32), meta(5, 2, 32, dtype=bf), meta(5, 2, 32), 8)),
        (RuntimeError, "unsupported dtype", lambda: A.check_shapes(meta(3, 2, 32, dtype=F64), meta(5, 2, 32, dtype=F64), meta(5, 2, 32, dtype=F64), 8)),
        (RuntimeError, "head dimension", lambda: devis_amd.multihead_attention(torch.zeros(3, 2, 24), torch.zeros(5, 2, 24), torch.zeros(5, 2, 24), 4)),
    ]
    for kind, match, call in bad:
        with pytest.raises(kind, match=match):
            call()
    # views: a last stride of 1 is passed through, anything else is made dense
    packed = torch.zeros(3, 2, 64)
    half = packed[..., 32:]
    assert A.as_view(half) is half and A.as_view(packed.transpose(0, 1)).stride() == (64, 128, 1)
    assert A.as_view(torch.zeros(3, 32, 2).transpose(1, 2)).is_contiguous()


# ---- the Function on the torch stand-in ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
def test_function_passes_gradcheck_in_float64(monkeypatch, p):
    import devis_amd
    fake_selfattn.install(monkeypatch)
    seed = torch.tensor([20260101], dtype=torch.int64) if p else None
    q, k, v = (rand(n, 2, 8, seed=i).requires_grad_(True) for i, n in enumerate((5, 7, 7)))
    assert torch.autograd.gradcheck(lambda *a: devis_amd.multihead_attention(*a, 2, p=p, seed=seed), (q, k, v))
    want = O.attention(q, k, v, 2, None if not p else O.keep_mask(20260101, 2, 2, 5, 7, p), O.scale_of(p))
    assert torch.allclose(devis_amd.multihead_attention(q, k, v, 2, p=p, seed=seed), want, atol=1e-12)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        out = devis_amd.multihead_attention(q, k, v, 2, p=p, seed=seed)
        gq, = torch.autograd.grad((out * out).sum(), v, create_graph=True)
        gq.sum().backward()


def test_function_computes_only_the_gradients_asked_for(monkeypatch):
    import devis_amd
    from devis_amd.functions import self_attention as A
    calls = fake_selfattn.install(monkeypatch)
    seed = torch.tensor([7], dtype=torch.int64)
    make = lambda: [rand(n, 2, 8, seed=i, dtype=F32) for i, n in enumerate((5, 7, 7))]      # noqa: E731
    ts = [t.requires_grad_(True) for t in make()]
    out = devis_amd.multihead_attention(*ts, 2, p=0.5, seed=seed)
    full = torch.autograd.grad((out * out).sum(), ts)
    del calls[:]
    with torch.no_grad():
        devis_amd.multihead_attention(*ts, 2)
    assert not devis_amd.multihead_attention(*make(), 2).requires_grad and calls == ["forward", "forward"]
    for asked in ((0,), (1,), (2,), (1, 2), (0, 2), (0, 1, 2)):
        ts = make()
        for i in asked:
            ts[i].requires_grad_(True)
        del calls[:]
        out = devis_amd.multihead_attention(*ts, 2, p=0.5, seed=seed)
        grads = torch.autograd.grad((out * out).sum(), [ts[i] for i in asked])
        for i, g in zip(asked, grads):
            assert torch.equal(g, full[i]) and g.dtype == ts[i].dtype and g.is_contiguous(), (asked, i)
        assert calls == ["forward", ("backward",) + tuple(i in asked for i in range(3))], (asked, calls)
    # the saved tensors: the operand views, out, lse and the seed -- no probabilities, no mask
    packed = rand(5, 2, 16, dtype=F32).requires_grad_(True)
    q, k, v = packed[..., :8], packed[..., 8:], make()[0].requires_grad_(True)
    out = A.MultiheadAttentionFunction.apply(q, k, v, seed, 2, 0.5)[0]
    saved = out.grad_fn.saved_tensors
    assert [tuple(t.shape) for t in saved] == [(5, 2, 8), (5, 2, 8), (5, 2, 8), (5, 2, 8), (4, 5), (1,)]
    assert saved[0].stride() == (32, 16, 1) and saved[0].data_ptr() == packed.data_ptr() and saved[4].dtype == F32
    # an empty key sequence: zeros, no launch
    del calls[:]
    empty = torch.zeros(0, 2, 8, requires_grad=True)
    out = devis_amd.multihead_attention(q, empty, empty, 2)
    gq, gk = torch.autograd.grad(out.sum(), (q, empty))
    assert not out.any() and out.shape == (5, 2, 8) and not gq.any() and gk.shape == (0, 2, 8) and calls == []
    assert devis_amd.multihead_attention(torch.zeros(0, 2, 8), v, v, 2).shape == (0, 2, 8) and calls == []


# ---- the module --------------------------------------------------------------------------------------------------------------

def modules(batch_first=False, dropout=0.0, E=32, H=8, seed=1, dtype=F64):
    import devis_amd
    torch.manual_seed(seed)
    stock = nn.MultiheadAttention(E, H, dropout=dropout, batch_first=batch_first).to(dtype).eval()
    with torch.no_grad():
        stock.in_proj_bias.normal_()
        stock.out_proj.bias.normal_()
    fused = devis_amd.FusedMultiheadAttention(E, H, dropout=dropout, batch_first=batch_first).to(dtype).eval()
    assert fused.load_state_dict(stock.state_dict()).missing_keys == [] and list(fused.state_dict()) == list(stock.state_dict())
    return stock, fused


@pytest.mark.parametrize("batch_first", [False, True])
@pytest.mark.parametrize("shared", [True, False])
def test_fused_module_equals_the_stock_module_in_float64(monkeypatch, batch_first, shared):
    calls = fake_selfattn.install(monkeypatch)
    stock, fused = modules(batch_first)
    L, S, N, E = (6, 6, 3, 32) if shared else (6, 9, 3, 32)
    shape = lambda rows: (N, rows, E) if batch_first else (rows, N, E)      # noqa: E731
    results = []
    for module in (stock, fused):
        x, key, value = rand(*shape(L), seed=3), rand(*shape(S), seed=4), rand(*shape(S), seed=5)
        leaves = [t.requires_grad_(True) for t in ((x, value) if shared else (x, key, value))]
        out, weights = module(x, x, value, need_weights=False) if shared else module(x, key, value, need_weights=False)
        assert weights is None
        params = list(module.parameters())
        results.append((out,) + torch.autograd.grad(out, leaves + params, rand(*shape(L), seed=6)))
    assert calls == ["forward", ("backward", True, True, True)]
    for a, b in zip(*results):
        assert a.shape == b.shape and float((a - b).detach().abs().max()) <= 1e-10
    # the fused projection split reproduces the packed one exactly enough: one linear for q and k when query is key
    linears = []
    real = F.linear
    monkeypatch.setattr(F, "linear", lambda x, w, b=None: linears.append(tuple(w.shape)) or real(x, w, b))
    x = rand(*shape(L), seed=3)
    fused(x, x, x, need_weights=False)
    assert linears == [(64, 32), (32, 32), (32, 32)]
    del linears[:]
    base = x.transpose(0, 1).contiguous()
    fused(base.transpose(0, 1), base.transpose(0, 1), x, need_weights=False)          # two equal views of one tensor
    assert linears == [(64, 32), (32, 32), (32, 32)]
    del linears[:]
    fused(x, rand(*shape(S), seed=4), rand(*shape(S), seed=5), need_weights=False)
    assert linears == [(32, 32)] * 4


def test_each_fallback_condition_reaches_the_stock_forward(monkeypatch):
    import devis_amd
    from devis_amd.modules import self_attention as M
    calls = fake_selfattn.install(monkeypatch)
    stock, fused = modules()
    x, y = rand(6, 3, 32, seed=3), rand(9, 3, 32, seed=4)
    want, want_weights = stock(x, x, x)

    def falls_back(module, *args, **kwargs):
        del calls[:]
        out = module(*args, **kwargs)
        assert calls == [], (args, kwargs)
        return out

    # need_weights (the default) without the flag: the stock result, weights included
    out, weights = falls_back(fused, x, x, x)
    assert torch.equal(out, want) and torch.equal(weights, want_weights)
    fused.discard_attention_weights = True
    del calls[:]
    out, weights = fused(x, x, x)
    assert weights is None and calls == ["forward"] and float((out - want).abs().max()) <= 1e-10
    # masks and causality
    pad = torch.zeros(3, 6, dtype=torch.bool)
    mask = torch.zeros(6, 6, dtype=torch.bool)
    assert torch.equal(falls_back(fused, x, x, x, key_padding_mask=pad)[0], want)
    assert torch.equal(falls_back(fused, x, x, x, attn_mask=mask)[0], want)
    causal = nn.Transformer.generate_square_subsequent_mask(6, dtype=F64)
    falls_back(fused, x, x, x, attn_mask=causal, is_causal=True)
    # unbatched input, key and value of different shapes (stock raises for the latter)
    assert falls_back(fused, x[:, 0], x[:, 0], x[:, 0])[0].shape == (6, 32)
    with pytest.raises((RuntimeError, AssertionError)):
        falls_back(fused, x, y, y[:5])
    # not on the GPU; compiling
    monkeypatch.setattr(M, "_on_gpu", lambda t: False)
    assert torch.equal(falls_back(fused, x, x, x)[0], want)
    monkeypatch.setattr(M, "_on_gpu", lambda t: True)
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    assert torch.equal(falls_back(fused, x, x, x)[0], want)
    monkeypatch.undo()
    calls = fake_selfattn.install(monkeypatch)
    # a dtype or a head dimension the kernels do not take
    monkeypatch.setattr(devis_amd.functions.self_attention, "DTYPES", (F32, torch.bfloat16, torch.float16))
    assert torch.equal(falls_back(fused, x, x, x)[0], want)                                # float64
    monkeypatch.setattr(devis_amd.functions.self_attention, "DTYPES", (F32, torch.bfloat16, torch.float16, F64))
    odd = devis_amd.FusedMultiheadAttention(12, 2).double().eval()                         # D = 6
    odd.discard_attention_weights = True
    falls_back(odd, rand(4, 1, 12), rand(4, 1, 12), rand(4, 1, 12))
    # other constructor options
    for kwargs in (dict(add_bias_kv=True), dict(add_zero_attn=True), dict(kdim=16, vdim=16)):
        other = devis_amd.FusedMultiheadAttention(32, 8, **kwargs).double().eval()
        other.discard_attention_weights = True
        kv = rand(6, 3, 16, seed=9) if "kdim" in kwargs else x
        assert falls_back(other, x, kv, kv)[0].shape == x.shape
    # no bias: fused
    plain = devis_amd.FusedMultiheadAttention(32, 8, bias=False).double().eval()
    ref = nn.MultiheadAttention(32, 8, bias=False).double().eval()
    ref.load_state_dict(plain.state_dict())
    del calls[:]
    assert float((plain(x, x, x, need_weights=False)[0] - ref(x, x, x)[0]).abs().max()) <= 1e-10 and calls == ["forward"]


def test_patch_sets_and_restores_the_exact_classes():
    import devis_amd
    from devis_amd.modules import self_attention as M

    class Mine(nn.MultiheadAttention):
        pass

    root = nn.ModuleDict({"a": nn.MultiheadAttention(32, 8), "b": nn.Sequential(nn.MultiheadAttention(16, 2, batch_first=True)),
                          "mine": Mine(32, 8), "lin": nn.Linear(4, 4)})
    keys = list(root.state_dict())
    previous = devis_amd.patch_self_attention(root)
    assert type(root["a"]) is type(root["b"][0]) is devis_amd.FusedMultiheadAttention and type(root["mine"]) is Mine
    assert root["a"].discard_attention_weights is True and list(root.state_dict()) == keys
    clone = copy.deepcopy(root["a"])
    assert type(clone) is devis_amd.FusedMultiheadAttention and clone.discard_attention_weights is True
    assert devis_amd.patch_self_attention(root) == []                                       # twice: nothing left to patch
    devis_amd.unpatch_self_attention(previous)
    assert type(root["a"]) is type(root["b"][0]) is nn.MultiheadAttention and M.FLAG not in root["a"].__dict__
    previous = devis_amd.patch_self_attention(root, discard_weights=False)
    assert root["a"].discard_attention_weights is False
    devis_amd.unpatch_self_attention(previous)
    assert type(root["a"]) is nn.MultiheadAttention and list(root.state_dict()) == keys
    assert "state dicts are untouched" in devis_amd.patch_self_attention.__doc__


def test_training_draws_one_seed_per_call_and_follows_manual_seed(monkeypatch):
    calls = fake_selfattn.install(monkeypatch)
    _, fused = modules(dropout=0.5)
    x = rand(6, 3, 32, seed=3)
    eval_out = fused(x, x, x, need_weights=False)[0]
    fused.train()
    drawn = []
    real = torch.randint
    monkeypatch.setattr(torch, "randint", lambda *a, **k: drawn.append(a) or real(*a, **k))
    torch.manual_seed(5)
    a = fused(x, x, x, need_weights=False)[0]
    assert len(drawn) == 1 and drawn[0][:3] == (-(1 << 63), (1 << 63) - 1, (1,))
    torch.manual_seed(5)
    b = fused(x, x, x, need_weights=False)[0]
    torch.manual_seed(6)
    c = fused(x, x, x, need_weights=False)[0]
    assert len(drawn) == 3 and torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, eval_out)
    assert calls == ["forward"] * 4


# ---- with the decoder layer --------------------------------------------------------------------------------------------------

def run_decoder(layer, inputs, attention, case):
    out = layer(*inputs)
    params = dict(layer.named_parameters())
    grads = torch.autograd.grad(out, [inputs[0], attention] + list(params.values()), case["grad_out"])
    got = {"out": out.detach(), "grad.tgt": grads[0], "grad.attention": grads[1]}
    got.update({"grad." + name: g for name, g in zip(params, grads[2:])})
    return got


def check_case(got, case, tol, what):
    wanted = [k for k in case if k == "out" or k.startswith("grad.")]
    assert sorted(got) == sorted(wanted), what
    assert sum(k.startswith("grad.self_attn.") for k in wanted) == 4
    for key in wanted:
        want = case[key]
        err, ref = float((got[key].detach().double().cpu() - want).abs().max()), float(want.abs().max())
        print("%s %s: max error %.3e, max |want| %.3e (tol %.0e)" % (what, key, err, ref, tol))
        assert err <= tol * ref, (what, key, err, ref)


@pytest.mark.parametrize("order", ["attention alone", "attention first", "layers first"])
def test_patched_decoder_layer_reproduces_the_reference_fixtures(monkeypatch, order):
    """The fixtures were recorded from the reference's decoder layer with a real nn.MultiheadAttention; they hold float64
    results rounded to float32, so 1e-6 of the largest value is the bar (tests/test_addnorm_cpu.py)."""
    import devis_amd
    from devis_amd.modules import transformer_layers as TL
    calls = fake_selfattn.install(monkeypatch)
    glue = fake_addnorm.install(monkeypatch)
    monkeypatch.setattr(TL, "_on_gpu", lambda x: True)
    case, module = LG.load_case("decoder"), LG.reference_module()
    layer, inputs, attention = LG.build_layer(module, "decoder", case)
    keys = list(layer.state_dict())
    undo_layers = None
    if order == "layers first":
        undo_layers = devis_amd.patch_transformer_layers(module)
    previous = devis_amd.patch_self_attention(layer)
    if order == "attention first":
        undo_layers = devis_amd.patch_transformer_layers(module)
    try:
        assert type(layer.self_attn) is devis_amd.FusedMultiheadAttention and list(layer.state_dict()) == keys
        check_case(run_decoder(layer, inputs, attention, case), case, 1e-6, order)
        assert calls == ["forward", ("backward", True, True, True)]
        assert (glue.count("forward") == 3) == (undo_layers is not None)
    finally:
        devis_amd.unpatch_self_attention(previous)
        if undo_layers is not None:
            devis_amd.unpatch_transformer_layers(module, undo_layers)
    assert type(layer.self_attn) is nn.MultiheadAttention
    del calls[:], glue[:]
    check_case(run_decoder(layer, inputs, attention, case), case, 1e-6, "unpatched")
    assert calls == [] and glue == []


# ---- the compiled path -----------------------------------------------------------------------------------------------------------

def test_compile_fullgraph_traces_the_stock_module_and_the_composite(monkeypatch):
    import devis_amd
    calls = fake_selfattn.install(monkeypatch)
    stock, fused = modules(dtype=F32)
    fused.discard_attention_weights = True
    x = rand(6, 3, 32, seed=3, dtype=F32)
    want = stock(x, x, x)[0]
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    try:
        torch._dynamo.reset()
        got = torch.compile(fused, fullgraph=True, backend=backend)(x, x, x)[0]
        assert torch.allclose(got, want, atol=1e-6) and calls == [] and len(graphs) == 1
        # the public function is the composite while compiling
        q, k, v = rand(5, 2, 8, seed=1, dtype=F32), rand(7, 2, 8, seed=2, dtype=F32), rand(7, 2, 8, seed=3, dtype=F32)
        f = torch.compile(lambda a, b, c: devis_amd.multihead_attention(a, b, c, 2), fullgraph=True, backend=backend)
        assert float((f(q, k, v).double() - O.attention(q, k, v, 2)).abs().max()) <= 1e-5 and calls == []
    finally:
        torch._dynamo.reset()


def test_the_namespace_has_no_new_op():
    import devis_amd  # noqa: F401
    from devis_amd import ops
    with open(os.path.join(ROOT, "tests", "golden", "op_schemas.json")) as f:
        want = json.load(f)
    prefix = ops.NAMESPACE + "::"
    names = sorted({n.split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith(prefix)})
    assert len(names) == len(want) == 34 and not any("attention" in n and "multihead" in n for n in names)
    assert not hasattr(ops, "multihead_attention") and "devis_amd.functions.self_attention" in sys.modules


# ---- the kernel variants and the inputs of the GPU tests (tests/selfattn_cases.py) -----------------------------------------------

def test_variant_of_restates_the_host_of_the_kernels():
    source = open(os.path.join(ROOT, "devis_amd", "csrc", "selfattn.hip")).read()
    # the three rules, where variant_of says they are: a change to either side fails here until the other follows
    assert source.count("switch ((D + 15) / 16)") == 1 and re.findall(r"Tiles<(\d)>\(\)\);", source) == ["1", "2", "3", "4"]
    assert source.count("const bool chunk_vec = pb.vec && (n & 3) == 0;") == 3 and source.count("D = pb.D, n = D >> 2;") == 3
    assert "bool quads(const selfattn_view &v) { return v.seq % 4 == 0 && v.batch % 4 == 0; }" in source
    assert "bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }" in source
    assert len(re.findall(r"const bool vec = aligned16\(q\) && aligned16\(k\) && aligned16\(v\) && aligned16\(out", source)) == 2
    assert [k for k in C.KERNELS if "void %s(" % k in source] == list(C.KERNELS)
    for name in ("dispatch_kernel", "selfattn_forward", "selfattn_backward", "chunk_vec"):
        assert name in C.variant_of.__doc__, name
    for dtype in C.DTYPES:
        assert [C.variant_of(D, dtype, True)[0] for D in range(4, 65, 4)] == [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4
        assert [D for D in range(4, 65, 4) if C.variant_of(D, dtype, True)[1]] == [16, 32, 48, 64]
        assert not any(any(C.variant_of(D, dtype, False)[1:]) for D in range(4, 65, 4))
    with pytest.raises(AssertionError):
        C.variant_of(32, F64, True)


@pytest.mark.parametrize("name", list(C.VIEWS))
def test_views_hold_equal_values_and_state_whether_the_call_is_vec(name):
    from devis_amd.functions import self_attention as A
    assert list(C.VIEWS) == ["dense", "packed", "batch_first", "shifted", "padded_rows", "only_v_unaligned", "broadcast"]
    view = C.VIEWS[name]
    for dtype in C.DTYPES:
        for L, S, N, H, D in ((5, 7, 2, 3, 4), (7, 5, 3, 1, 4), (1, 1, 1, 1, 4), (6, 6, 1, 2, 16), (3, 9, 4, 1, 20)):
            dense = C.make_inputs(L, S, N, H, D, dtype)
            got = view.build(*dense)
            want = dense if name != "broadcast" else tuple(t[:, :1].expand_as(t) for t in dense[:3]) + dense[3:]
            for a, b in zip(got, want):
                assert a.shape == b.shape and a.dtype == dtype and torch.equal(a, b) and A.as_view(a) is a, (name, dtype)
            assert C.aligned_and_quad_strided(*got) is view.vec(H * D, dtype), (name, dtype, L, S, N, H, D)
            if name == "broadcast" and N > 1:
                assert all(t.stride(1) == 0 for t in got[:3])
    assert C.VIEWS["packed"].vec(4, torch.bfloat16) is False and C.VIEWS["packed"].vec(4, F32) is True


def test_the_sweep_and_the_matrices_reach_every_compiled_variant():
    """A condition on the generator and on the parameter lists, not a measurement."""
    configs = [C.sweep_config(seed) for seed in C.SWEEP]
    assert len(configs) == 96 and configs == [C.sweep_config(seed) for seed in C.SWEEP]
    reached, views, vecs = collections.Counter(), collections.Counter(), set()
    for c in configs:
        assert 1 <= c.L <= 80 and 1 <= c.S <= 80 and 1 <= c.N <= 3 and 1 <= c.H <= 4 and c.D in range(4, 65, 4)
        assert c.p in (0.0, 0.1, 0.5) and c.dtype in C.DTYPES and c.view in C.VIEWS and -(1 << 63) <= c.dropout_seed < 1 << 63
        ct, chunk, vec = C.variant_of(c.D, c.dtype, C.VIEWS[c.view].vec(c.H * c.D, c.dtype))
        reached[c.dtype, ct, c.D % 16 == 0] += 1
        views[c.view] += 1
        vecs.add((c.dtype, vec, chunk))
    assert sorted(reached, key=str) == sorted(C.classes(), key=str) and len(reached) == 24 and min(reached.values()) >= 2, reached
    assert sorted(views) == sorted(C.VIEWS) and min(views.values()) >= 5, views
    for dtype in C.DTYPES:                   # per element; vector stores with per-element chunks; vector everything
        assert {(vec, chunk) for d, vec, chunk in vecs if d is dtype} == {(False, False), (True, False), (True, True)}, dtype
    assert {c.p for c in configs} == {0.0, 0.1, 0.5} and len({c.D for c in configs}) == 16
    # the head-dimension matrices launch each of the 36 instantiations and compare it with the oracle
    want = {(kernel, dtype, ct) for kernel in C.KERNELS for dtype in C.DTYPES for ct in (1, 2, 3, 4)}
    assert C.oracle_matrix_variants() == want and len(want) == 36
    # the view matrix compares both load paths of every (dtype, CT) bit for bit: "dense" is vec, "shifted" is not
    both = {(dtype, C.variant_of(D, dtype, True)[0]) for D, dtype in C.VIEW_MATRIX}
    assert both == {(dtype, ct) for dtype in C.DTYPES for ct in (1, 2, 3, 4)}
    assert {C.variant_of(D, dtype, True)[1] for D, dtype in C.VIEW_MATRIX} == {True, False}
    E = [C.VIEW_SHAPE[3] * D for D, _ in C.VIEW_MATRIX]
    assert all(C.VIEWS["dense"].vec(e, F32) for e in E) and not any(C.VIEWS["shifted"].vec(e, F32) for e in E)
    # the lists are what the issue sets
    assert len(C.MATRIX_F32) == 32 and len(C.MATRIX_16) == 36 and len(C.PLANTED) == 48 and len(C.LOPSIDED) == 8


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_the_backward_takes_out_in_float32_before_its_rounding(monkeypatch, dtype):
    """delta = sum(dO * O) cancels against dP in dS = P (dP - delta): with O rounded to bfloat16 a peaked softmax left grad_q and
    grad_k off by up to 10 % of their maximum.  The forward writes a float32 copy for the backward of 16-bit operands."""
    from devis_amd import _selfattn
    from devis_amd.functions import self_attention as A
    fake_selfattn.install(monkeypatch)
    counts, double = [], _selfattn.forward
    monkeypatch.setattr(_selfattn, "forward", lambda *a: counts.append(len(a)) or double(*a))
    q, k, v, go = (t.requires_grad_(True) for t in C.make_inputs(5, 7, 2, 2, 8, dtype))
    out, lse, acc = A.MultiheadAttentionFunction.apply(q, k, v, None, 2, 0.0)
    assert counts == [9 if dtype == F32 else 10]          # float32: the call as it was before out_acc, for older doubles
    saved = out.grad_fn.saved_tensors
    assert out.dtype == dtype and saved[3].dtype == F32 and lse.dtype == F32 and not lse.requires_grad
    if dtype == F32:
        assert acc is None and saved[3].data_ptr() == out.data_ptr()
    else:
        assert saved[3].data_ptr() == acc.data_ptr() and not acc.requires_grad and torch.equal(acc.to(dtype), out)
        assert not torch.equal(acc, out.float())
    with torch.no_grad():
        assert A._forward(q, k, v, None, 2, 0.0, want_lse=False)[1:] == (None, None)
    monkeypatch.undo()
    if dtype != F32:                            # the binding refuses the rounded out before any call
        with pytest.raises(RuntimeError, match="must be float32"):
            _selfattn.backward(2, q, k, v, out.detach(), go, lse, None, 0.0, _selfattn.Shape(5, 7, 2, 16, 2), None, None, None)


def double_shares(operands, H, D, dtype, p, seed, cancelling=()):
    """{tensor: max|double - oracle| as a share of max|oracle|} of the CPU double (tests/fake_selfattn.py, installed by the
    caller) on ``operands``; for the tensors in ``cancelling`` and beside an all-zero oracle the share is of the cancelling
    terms, as in tests/test_selfattn_gpu.py::compare."""
    dense = [t.contiguous() for t in operands]
    L, N, S = dense[0].shape[0], dense[0].shape[1], dense[1].shape[0]
    keep = None if not p else O.keep_mask(seed, N, H, L, S, p)
    want = O.attention_grads(*dense[:3], H, dense[3], keep, O.scale_of(p))
    got = C.run(*operands, H, p, None if not p else torch.tensor([seed], dtype=torch.int64))
    shares = {}
    for name, a, b in zip(C.NAMES, got, want):
        assert a.dtype == dtype and a.shape == b.shape and bool(a.isfinite().all()), name
        ref = float(b.abs().max())
        if name in cancelling or ref == 0.0:
            ref = C.cancelling_terms(*dense, D, p)
        shares[name] = float((a.double() - b).abs().max()) / ref
    return shares


def double_cases(group):
    """(what, operands, H, D, dtype, p, seed, cancelling) of every case of a group of GPU tests."""
    if group == "sweep":
        for seed in C.SWEEP:
            c = C.sweep_config(seed)
            operands = C.VIEWS[c.view].build(*C.make_inputs(c.L, c.S, c.N, c.H, c.D, c.dtype, seed=seed))
            yield str(c), operands, c.H, c.D, c.dtype, c.p, c.dropout_seed, ()
    elif group == "float32 matrix":
        for L, S, N, H, D in C.MATRIX_F32:
            yield str((L, S, D)), C.make_inputs(L, S, N, H, D), H, D, F32, 0.0, None, ()
    elif group == "16-bit matrix":
        for L, S, N, H, D, dtype, p in C.MATRIX_16:
            yield str((D, dtype, p)), C.make_inputs(L, S, N, H, D, dtype), H, D, dtype, p, C.DROPOUT_SEED, ()
    elif group == "views":
        L, S, N, H = C.VIEW_SHAPE
        for D, dtype in C.VIEW_MATRIX:
            yield str((D, dtype)), C.make_inputs(L, S, N, H, D, dtype), H, D, dtype, 0.5, C.DROPOUT_SEED, ()
    elif group == "planted maxima":
        L, N, H, D = C.PLANTED_SHAPE
        for S, dtype, p, last, boost in C.PLANTED:
            operands = C.planted_inputs(L, S, N, H, D, dtype, S - 1 if last else 0, boost)
            yield str((S, dtype, p, last, boost)), operands, H, D, dtype, p, C.DROPOUT_SEED, ("grad_q", "grad_k") if boost > 9 else ()
    elif group == "lopsided":
        for L, S, N, H, D, p in C.LOPSIDED:
            yield str((L, S, p)), C.make_inputs(L, S, N, H, D), H, D, F32, p, C.DROPOUT_SEED, ()


@pytest.mark.parametrize("group", ["sweep", "float32 matrix", "16-bit matrix", "views", "planted maxima", "lopsided"])
def test_the_inputs_leave_a_correct_implementation_inside_half_of_each_bar(monkeypatch, group):
    """Every input the GPU tests feed the kernels, through the CPU double -- float32 arithmetic on the rounded operands, results
    rounded once -- against the float64 oracle: at most HALF of the bar of tests/test_selfattn_gpu.py for each tensor, so that a
    kernel that misses a bar there is wrong and not unlucky.  Worst shares of max|want| as printed below, float32 / bfloat16 /
    float16: sweep 7.2e-7 / 3.7e-3 / 4.5e-4; the matrices 6.6e-7 / 3.5e-3 / 4.6e-4; views 4.1e-7 / 3.2e-3 / 3.9e-4; planted maxima
    9.2e-6 / 3.1e-3 / 3.9e-4; lopsided 6.5e-7 -- 37 % of a bar at most, so the generator needed no restriction.  (With the
    backward reading the rounded out, as it did, the planted maxima gave 9.5e-2 in bfloat16 and 1.0e-2 in float16.)"""
    from test_attmap_gpu import TOL
    fake_selfattn.install(monkeypatch)
    worst = {}
    for what, operands, H, D, dtype, p, seed, cancelling in double_cases(group):
        for name, share in double_shares(operands, H, D, dtype, p, seed, cancelling).items():
            if share > worst.get(dtype, (0.0,))[0]:
                worst[dtype] = (share, name, what)
            assert share <= 0.5 * TOL[dtype], (what, name, share)
    for dtype, (share, name, what) in worst.items():
        print("%s %s: the double's worst error %.2e of max |want| (%s of %s), bar %.0e" % (group, dtype, share, name, what, TOL[dtype]))


# ---- documents ---------------------------------------------------------------------------------------------------------------

def test_the_documents_describe_the_operator():
    import devis_amd
    read = lambda name: open(os.path.join(ROOT, name)).read()      # noqa: E731
    design, integration, readme = read("DESIGN.md"), read("INTEGRATION.md"), read("README.md")
    assert re.search(r"^## 20\. .*self-attention", design, re.M)
    section = design.split("## 20.")[1]
    for phrase in ("Philox4x32-10", "torch.library", "launches", "transposed", "lse", "v_mfma_f32_16x16x4_f32", "1e-4"):
        assert phrase in section, phrase
    assert re.search(r"^#+ Transformer layers: decoder self-attention", integration, re.M)
    part = integration.split("Transformer layers: decoder self-attention")[1]
    for phrase in ("patch_self_attention", "discard_weights", "key_padding_mask", "is_compiling", "torch.randint", "Not implemented on the CPU"):
        assert phrase in part, phrase
    assert "the attention inside `nn.MultiheadAttention`" not in integration
    assert "multihead_attention" in readme and "selfattn.h" in readme and "self_attention.py" in readme
    assert "selfattn.h" in devis_amd.__doc__ and "multihead_attention" in devis_amd.__doc__
    assert os.path.exists(os.path.join(ROOT, "scripts", "selfattn_bench.py"))
    if not os.path.exists(os.path.join(ROOT, "profiles", "selfattn_bench.json")):
        assert "no ratio is quoted" in readme and "not measured" in readme
