"""CPU tests of the transformer layers' glue operators: the oracle (Philox known answers, the reference fixtures), the C ABI of
include/addnorm.h (exports, version, argument errors -- no compute calls), the host code (checks, errors, which gradients are
computed) with the binding replaced by the torch stand-in of tests/fake_addnorm.py, the patch on stand-in and on the real
reference classes, and the compiled path.  The kernels themselves are tests/test_addnorm_gpu.py."""
import ctypes
import os
import re
import sys
import types

import pytest
import torch
import torch.nn.functional as F

import addnorm_oracle as O
import fake_addnorm
import layerglue_cases as L
from conftest import ROOT, golden_names

F32, F64 = torch.float32, torch.float64
REF_SRC = "/root/reference/src"


# ---- oracle ------------------------------------------------------------------------------------------------------------------

def test_philox_reproduces_the_published_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    for counter, key, want in (
            ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
            ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")):
        assert " ".join("%08x" % int(w) for w in O.philox4x32_10(counter, key)) == want


def test_keep_mask_follows_the_rule_of_the_header():
    seed, R, C = 0x123456789ABCDEF, 3, 7
    keep = O.keep_mask(seed, R, C, 0.5)
    assert keep.shape == (R, C) and keep.dtype == torch.bool
    for row, c in ((0, 0), (1, 3), (2, 4), (2, 6)):
        words = O.philox4x32_10((row, 0, c >> 2, 0), (seed & 0xffffffff, seed >> 32))
        assert bool(keep[row, c]) == (int(words[c & 3]) >= 1 << 31)
    assert O.keep_mask(seed, R, C, 0.0).all() and not O.keep_mask(seed, R, C, 1.0).any()
    assert O.threshold_of(1.0) == 1 << 32 and O.threshold_of(0.1) == 429496729 and O.scale_of(1.0) == 0.0
    assert torch.equal(O.keep_mask(-1, R, C, 0.5), O.keep_mask((1 << 64) - 1, R, C, 0.5))             # int64 -1: all key bits
    assert not torch.equal(O.keep_mask(1, 4, 64, 0.5), O.keep_mask(1 << 32, 4, 64, 0.5))              # the high word counts


def oracle_layer(kind, layer, inputs):
    """The layer's chain with the glue computed by the oracle (float64)."""
    site = lambda x, delta, norm: O.add_layer_norm(x, delta, norm.weight, norm.bias, norm.eps)      # noqa: E731
    if kind == "encoder":
        src, pos = inputs[:2]
        x = site(src, layer.self_attn(src + pos)[0], layer.norm1)
        return site(x, layer.linear2(O.relu_dropout(layer.linear1(x))), layer.norm2)
    tgt, query_pos = inputs[:2]
    q = (tgt + query_pos).transpose(0, 1)
    x = site(tgt, layer.self_attn(q, q, tgt.transpose(0, 1))[0].transpose(0, 1), layer.norm2)
    x = site(x, layer.cross_attn(x + query_pos)[0], layer.norm1)
    return site(x, layer.linear2(O.relu_dropout(layer.linear1(x))), layer.norm3)


def check_case(got, case, tol, what):
    """Every recorded result: max|got - want| <= tol * max|want|."""
    wanted = [k for k in case if k == "out" or k.startswith("grad.")]
    assert sorted(got) == sorted(wanted), what
    for key in wanted:
        want = case[key]
        err, ref = float((got[key].detach().double().cpu() - want).abs().max()), float(want.abs().max())
        print("%s %s: max error %.3e, max |want| %.3e (tol %.0e)" % (what, key, err, ref, tol))
        assert err <= tol * ref, (what, key, err, ref)


def test_fixtures_cover_the_cases():
    assert golden_names("layerglue_") == ["layerglue_decoder", "layerglue_decoder_grads_attention", "layerglue_decoder_grads_ffn",
                                          "layerglue_encoder", "layerglue_encoder_grads"]
    for name in golden_names("layerglue_"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 32 << 10
    enc, dec = L.load_case("encoder"), L.load_case("decoder")
    assert tuple(enc["src"].shape) == (2, 7, 32) and tuple(dec["tgt"].shape) == (1, 6, 32)
    assert tuple(enc["state.linear1.weight"].shape) == (64, 32) and "state.self_attn.in_proj_weight" in dec
    for case in (enc, dec):
        params = [k[len("state."):] for k in case if k.startswith("state.")]
        assert all("grad." + name in case for name in params) and "grad.attention" in case and "out" in case


@pytest.mark.parametrize("kind", ["encoder", "decoder"])
def test_oracle_and_stand_in_layers_reproduce_the_reference_fixtures(kind):
    """The fixtures hold float64 results rounded to float32: 2^-24, so 1e-6 of the largest value is the bar."""
    case = L.load_case(kind)
    module = L.reference_module()
    check_case(L.run_case(module, kind, case), case, 1e-6, "stand-in " + kind)
    layer, inputs, attention = L.build_layer(module, kind, case)
    out = oracle_layer(kind, layer, inputs)
    params = dict(layer.named_parameters())
    grads = torch.autograd.grad(out, [inputs[0], attention] + list(params.values()), case["grad_out"])
    got = {"out": out, "grad." + ("src" if kind == "encoder" else "tgt"): grads[0], "grad.attention": grads[1]}
    got.update({"grad." + name: g for name, g in zip(params, grads[2:])})
    check_case(got, case, 1e-6, "oracle " + kind)


# ---- library -----------------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_addnorm_h_declares_and_versions_agree():
    from devis_amd import _addnorm, _native, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "addnorm.h")).read()
    declared = set(re.findall(r"\b(addnorm_[a-z_0-9]+)\s*\(", header.split("#ifndef ADDNORM_H")[1]))
    assert declared == set(_addnorm.EXPORTED_SYMBOLS) and len(declared) == 8
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _addnorm.load()
    assert lib.addnorm_version() == _addnorm.ADDNORM_ABI_VERSION == 1 == int(re.search(r"#define ADDNORM_ABI_VERSION (\d+)", header).group(1))
    assert dict(re.findall(r"ADDNORM_(F32|F64|BF16|F16) = (\d)", header)) == {"F32": "0", "F64": "1", "BF16": "2", "F16": "3"}
    for name, value in (("TILE_ROWS", _addnorm.TILE_ROWS), ("TILE_CHANNELS", _addnorm.TILE_CHANNELS), ("MAX_CHANNELS", _addnorm.MAX_CHANNELS)):
        assert int(re.search(r"#define ADDNORM_%s (\d+)" % name, header).group(1)) == value, name
    assert _addnorm.tile(_addnorm.TILE_ROWS) > 0 and _addnorm.tile(_addnorm.TILE_CHANNELS) == 1024
    assert lib.addnorm_tile(2) == -1 and lib.addnorm_tile(-1) == -1
    assert ctypes.sizeof(_addnorm.Shape) == 16 and ctypes.sizeof(_addnorm.Types) == 16
    assert _native.load().msda_build_info().decode() == "abi=14 arch=gfx950"              # no other ABI moved
    assert os.path.join(build.include_dir(), "addnorm.h") in build._headers()
    assert any(s.endswith("addnorm.hip") for s in build.sources())
    assert "addnorm.h" in open(os.path.join(ROOT, "setup.py")).read() and "addnorm.h" in build.include_dir.__doc__
    for phrase in ("Philox4x32-10", "row >> 32", "c >> 2", "floor(p * 2^32)", "implies y > 0"):
        assert phrase in header, phrase


def test_addnorm_argument_errors_without_gpu():
    from devis_amd import _addnorm
    lib = _addnorm.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.addnorm_last_error
    shape = lambda R=5, C=32: ctypes.byref(_addnorm.Shape(R, C))                       # noqa: E731
    types_ = lambda x=0, d=0, y=0, w=0: ctypes.byref(_addnorm.Types(x, d, y, w))       # noqa: E731
    fwd = lambda t=types_(), x=p, d=p, w=p, b=p, seed=p, pr=0.1, eps=1e-5, s=shape(), y=p, m=p, r=p: lib.addnorm_forward(      # noqa: E731
        t, x, d, w, b, seed, pr, eps, s, y, m, r, None)
    bwd = lambda t=types_(), x=p, d=p, w=p, seed=p, pr=0.1, m=p, r=p, g=p, s=shape(), ws=p, gx=p, gd=p, gw=p, gb=p: lib.addnorm_backward(      # noqa: E731
        t, x, d, w, seed, pr, m, r, g, s, ws, gx, gd, gw, gb, None)
    relu = lambda dt=0, x=p, seed=p, pr=0.1, s=shape(), y=p: lib.addnorm_relu_forward(dt, x, seed, pr, s, y, None)      # noqa: E731
    rbwd = lambda dt=0, y=p, g=p, pr=0.1, n=8, gx=p: lib.addnorm_relu_backward(dt, y, g, pr, n, gx, None)               # noqa: E731
    for call in (fwd, bwd):
        assert call(t=None) == -1 and b"null pointer" in err()
        assert call(t=types_(x=9)) == -1 and b"dtype" in err()
        for bad in ((0, 1, 0, 0), (1, 0, 1, 1), (0, 0, 2, 0), (2, 3, 2, 2), (2, 2, 3, 2), (0, 2, 0, 2), (0, 0, 0, 2), (1, 1, 1, 0), (2, 2, 2, 3)):
            assert call(t=types_(*bad)) == -1 and b"unsupported combination" in err(), bad
        assert call(s=shape(C=1025)) == -1 and b"channels" in err()
    for call in (fwd, bwd, relu):
        assert call(s=None) == -1 and b"null pointer" in err()
        assert call(s=shape(R=-1)) == -1 and b"negative" in err()
        assert call(s=shape(R=1 << 31)) == -1 and b"31 bits" in err()
        assert call(s=shape(C=0)) == -1 and b"positive" in err()
        assert call(seed=None) == -1 and b"seed is required" in err()
    for call in (fwd, bwd, relu, rbwd):
        for bad in (-0.1, 1.5, float("nan")):
            assert call(pr=bad) == -1 and b"[0, 1]" in err()
    assert fwd(eps=float("nan")) == -1 and b"eps" in err()
    for name in ("x", "d", "w", "b", "y"):
        assert fwd(**{name: None}) == -1 and b"null pointer" in err(), name
    assert fwd(m=None) == -1 and b"together" in err() and fwd(r=None) == -1
    assert bwd(gx=None, gd=None, gw=None, gb=None) == -1 and b"no gradient" in err()
    for name in ("x", "d", "m", "r", "g"):
        assert bwd(**{name: None}) == -1 and b"null pointer" in err(), name
    assert bwd(w=None) == -1 and b"weight" in err()
    rows = lib.addnorm_tile(0)
    assert bwd(s=shape(R=rows + 1), ws=None) == -1 and b"workspace" in err()
    assert bwd(ws=ctypes.c_void_p(p.value + 4)) == -1 and b"16-byte" in err()
    assert relu(dt=7) == -1 and b"dtype" in err() and relu(x=None) == -1 and b"null pointer" in err()
    assert rbwd(dt=7) == -1 and rbwd(n=-1) == -1 and b"negative" in err() and rbwd(y=None) == -1 and b"null pointer" in err()
    # nothing to compute: nothing is launched, nothing is dereferenced
    assert fwd(x=None, d=None, w=None, b=None, y=None, m=None, r=None, s=shape(R=0)) == 0
    assert bwd(x=None, d=None, w=None, m=None, r=None, g=None, ws=None, s=shape(R=0)) == 0
    assert relu(x=None, y=None, s=shape(R=0)) == 0 and rbwd(y=None, g=None, gx=None, n=0) == 0
    # the workspace: host arithmetic
    ws = lambda dt=0, **kw: lib.addnorm_workspace_bytes(dt, shape(**kw))      # noqa: E731
    assert ws(R=rows) == 0 and ws(R=1) == 0 and ws(R=0) == 0
    assert ws(R=rows + 1, C=32) == 2 * 2 * 32 * 4 and ws(1, R=rows + 1, C=32) == 2 * 2 * 32 * 8
    assert ws(R=3 * rows, C=7) == 256 and ws(R=3 * rows, C=7) >= 3 * 2 * 7 * 4
    assert ws(9) == -1 and b"dtype" in err() and ws(C=1025) == -1 and lib.addnorm_workspace_bytes(0, None) == -1


def test_operators_raise_on_cpu_tensors_and_on_bad_arguments_before_any_launch(monkeypatch):
    import devis_amd
    from devis_amd import _addnorm
    from devis_amd.functions import add_norm as A

    def no_launch(*a, **k):
        raise AssertionError("a kernel call was made")

    for name in ("forward", "backward", "relu_forward", "relu_backward"):
        monkeypatch.setattr(_addnorm, name, no_launch)
    x, w, seed = torch.zeros(2, 3, 8), torch.ones(8), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.add_layer_norm(x, x, w, w)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.add_layer_norm(x.requires_grad_(True), x, w, w, p=0.5, seed=seed)
    x = x.detach()
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.relu_dropout(x)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        A._backward(x, x, x, w, torch.zeros(2, 3), torch.zeros(2, 3), None, 0.0, (True, True, True, True))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        A._relu_backward(x, x, 0.0)
    for name in ("add_layer_norm", "relu_dropout", "patch_transformer_layers", "unpatch_transformer_layers"):
        assert name in devis_amd.__all__ and hasattr(devis_amd, name)
    assert devis_amd.add_layer_norm is A.add_layer_norm and devis_amd.relu_dropout is A.relu_dropout
    assert devis_amd.patch_transformer_layers is devis_amd.argument_builders.patch_transformer_layers
    assert "no CPU path" in A.__doc__ and "IGNORES ``seed``" in A.__doc__

    meta = lambda *s, dtype=F32: torch.zeros(*s, dtype=dtype, device="meta")      # noqa: E731
    bf, f16 = torch.bfloat16, torch.float16
    assert A.check_norm(meta(2, 3, 8), meta(2, 3, 8), meta(8), meta(8), None) == (6, 8, F32)
    assert A.check_norm(meta(8), meta(8), meta(8), meta(8), None) == (1, 8, F32)
    assert A.check_norm(meta(0, 8), meta(0, 8), meta(8), meta(8), None) == (0, 8, F32)
    assert A.check_norm(meta(4, 1024, dtype=bf), meta(4, 1024, dtype=bf), meta(1024), meta(1024), F32) == (4, 1024, F32)
    good = [(F32, F32, F32, None), (F64, F64, F64, None), (bf, bf, bf, None), (f16, f16, f16, None), (bf, bf, F32, None),
            (f16, f16, F32, None), (F32, bf, F32, None), (F32, f16, F32, None), (bf, bf, bf, F32), (f16, f16, F32, F32), (F32, F32, F32, F32)]
    for combo in good:
        assert A.supported(*combo), combo
    for combo in [(F32, F64, F32, None), (F64, F32, F64, None), (bf, f16, bf, None), (bf, F32, bf, None), (F32, bf, bf, None),
                  (F32, F32, bf, None), (F64, F64, F32, None), (F32, F32, F32, bf), (F64, F64, F64, F32), (bf, bf, bf, f16),
                  (torch.int32, torch.int32, F32, None)]:
        assert not A.supported(*combo), combo
    bad = [
        (ValueError, "between 0 and 1", lambda: devis_amd.add_layer_norm(x, x, w, w, p=1.5, seed=seed)),
        (ValueError, "between 0 and 1", lambda: devis_amd.add_layer_norm(x, x, w, w, p=-0.1)),
        (ValueError, "between 0 and 1", lambda: devis_amd.relu_dropout(x, p=float("nan"), seed=seed)),
        (ValueError, "needs a seed", lambda: devis_amd.add_layer_norm(x, x, w, w, p=0.1)),
        (ValueError, "needs a seed", lambda: devis_amd.relu_dropout(x, p=1.0)),
        (RuntimeError, "int64 tensor of one element", lambda: devis_amd.relu_dropout(x, p=0.5, seed=torch.zeros(1))),
        (RuntimeError, "int64 tensor of one element", lambda: devis_amd.add_layer_norm(x, x, w, w, p=0.5, seed=torch.zeros(2, dtype=torch.int64))),
        (RuntimeError, "1 to 1024 channels, got 1025", lambda: A.check_norm(meta(2, 1025), meta(2, 1025), meta(1025), meta(1025), None)),
        (RuntimeError, "1 to 1024 channels, got 0", lambda: A.check_norm(meta(2, 0), meta(2, 0), meta(0), meta(0), None)),
        (RuntimeError, "one shape", lambda: A.check_norm(meta(2, 8), meta(3, 8), meta(8), meta(8), None)),
        (RuntimeError, "one shape", lambda: A.check_norm(meta(()), meta(()), meta(8), meta(8), None)),
        (RuntimeError, "weight and bias are required", lambda: A.check_norm(meta(2, 8), meta(2, 8), None, None, None)),
        (RuntimeError, r"must be \[8\]", lambda: A.check_norm(meta(2, 8), meta(2, 8), meta(4), meta(8), None)),
        (RuntimeError, "weight is", lambda: A.check_norm(meta(2, 8), meta(2, 8), meta(8), meta(8, dtype=F64), None)),
        (RuntimeError, "unsupported dtypes", lambda: A.check_norm(meta(2, 8), meta(2, 8, dtype=F64), meta(8), meta(8), None)),
        (RuntimeError, "unsupported dtypes", lambda: A.check_norm(meta(2, 8), meta(2, 8), meta(8), meta(8), bf)),
        (RuntimeError, "unsupported dtype", lambda: devis_amd.relu_dropout(torch.zeros(2, 8, dtype=torch.int32))),
        (RuntimeError, "1 to 1024 channels", lambda: devis_amd.add_layer_norm(torch.zeros(2, 1025), torch.zeros(2, 1025), torch.ones(1025), torch.ones(1025))),
    ]
    for kind, match, call in bad:
        with pytest.raises(kind, match=match):
            call()
    # p == 0: the seed is ignored, whatever it is
    assert A.check_p("x", 0, "anything") == 0.0 and A.check_p("x", 1, seed) == 1.0


# ---- the Functions on the torch stand-in ----------------------------------------------------------------------------------------

def leaves(R=5, C=12, dtype=F64, seed=3):
    g = torch.Generator().manual_seed(seed)
    x, delta = torch.randn(2, R, C, generator=g, dtype=dtype), torch.randn(2, R, C, generator=g, dtype=dtype)
    weight, bias = torch.randn(C, generator=g, dtype=dtype) + 1, torch.randn(C, generator=g, dtype=dtype)
    return [t.requires_grad_(True) for t in (x, delta, weight, bias)]


@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
def test_functions_pass_gradcheck_in_float64(monkeypatch, p):
    import devis_amd
    fake_addnorm.install(monkeypatch)
    seed = torch.tensor([20260101], dtype=torch.int64) if p else None
    x, delta, weight, bias = leaves()
    assert torch.autograd.gradcheck(lambda *a: devis_amd.add_layer_norm(*a, 1e-5, p=p, seed=seed), (x, delta, weight, bias))
    want = O.add_layer_norm(x, delta, weight, bias, 1e-5, None if not p else O.keep_mask(20260101, 10, 12, p), O.scale_of(p))
    assert torch.allclose(devis_amd.add_layer_norm(x, delta, weight, bias, p=p, seed=seed), want, atol=1e-12)
    h = x.detach().clone()
    h[h.abs() < 0.05] = 0.5                              # away from the kink
    h.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a: devis_amd.relu_dropout(a, p=p, seed=seed), (h,))
    want = O.relu_dropout(h, None if not p else O.keep_mask(20260101, 10, 12, p), O.scale_of(p))
    assert torch.allclose(devis_amd.relu_dropout(h, p=p, seed=seed), want, atol=1e-12)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        y = devis_amd.relu_dropout(h, p=p, seed=seed) + devis_amd.add_layer_norm(x, delta, weight, bias, p=p, seed=seed)
        gx, = torch.autograd.grad((y * y).sum(), h if p < 1 else x, create_graph=True)
        gx.sum().backward()


def test_functions_compute_only_the_gradients_asked_for(monkeypatch):
    import devis_amd
    from devis_amd.functions import add_norm as A
    calls = fake_addnorm.install(monkeypatch)
    seed = torch.tensor([7], dtype=torch.int64)
    full = {}
    for p in (0.0, 0.5, 1.0):
        x, delta, weight, bias = leaves(dtype=F32)
        y = devis_amd.add_layer_norm(x, delta, weight, bias, p=p, seed=seed if p else None)
        full[p] = torch.autograd.grad(y.sum() + (y * y).sum(), (x, delta, weight, bias))
    # no gradient: no statistics, no Function, no backward
    del calls[:]
    with torch.no_grad():
        devis_amd.add_layer_norm(*leaves(dtype=F32))
    y = devis_amd.add_layer_norm(*(t.detach() for t in leaves(dtype=F32)))
    assert not y.requires_grad and calls == ["forward", "forward"]
    for p in (0.0, 0.5, 1.0):
        for asked in ((0,), (1,), (2,), (3,), (0, 1), (2, 3), (1, 3), (0, 1, 2, 3)):
            ts = [t.detach() for t in leaves(dtype=F32)]
            for i in asked:
                ts[i].requires_grad_(True)
            del calls[:]
            y = devis_amd.add_layer_norm(*ts, p=p, seed=seed if p else None)
            grads = torch.autograd.grad(y.sum() + (y * y).sum(), [ts[i] for i in asked])
            for i, g in zip(asked, grads):
                assert torch.equal(g, full[p][i]) and g.dtype == ts[i].dtype, (p, asked, i)
            want_x, want_d, want_w, want_b = (i in asked for i in range(4))
            if p == 0.0:                                             # grad_delta is grad_x
                expect = [("backward", want_x or want_d, False, want_w, want_b)]
            elif p == 1.0:                                           # grad_delta is zeros: no launch of its own
                expect = [("backward", want_x, False, want_w, want_b)] if want_x or want_w or want_b else []
                if want_d:
                    assert not grads[asked.index(1)].any()
            else:
                expect = [("backward", want_x, want_d, want_w, want_b)]
            assert calls == ["forward"] + expect, (p, asked, calls)
    # a mixed call writes grad_delta in delta's dtype from the kernel
    x, delta, weight, bias = leaves(dtype=F32)
    half = delta.detach().to(torch.bfloat16).requires_grad_(True)
    del calls[:]
    gx, gd = torch.autograd.grad(devis_amd.add_layer_norm(x, half, weight.detach(), bias.detach()).sum(), (x, half))
    assert gd.dtype == torch.bfloat16 and gx.dtype == F32 and calls[-1] == ("backward", True, True, False, False)
    # the saved tensors: the operands, the statistics and the seed -- not y, not the sum, no mask
    y = A.AddLayerNormFunction.apply(x, delta, weight, bias, seed, 1e-5, 0.5, None)[0]
    saved = y.grad_fn.saved_tensors
    assert len(saved) == 6 and [tuple(t.shape) for t in saved] == [(2, 5, 12), (2, 5, 12), (12,), (2, 5), (2, 5), (1,)]
    assert saved[0] is x and saved[1] is delta and saved[5].dtype == torch.int64
    # the relu pass saves y alone and launches nothing when no gradient is asked for
    h = x.detach().requires_grad_(True)
    del calls[:]
    out = devis_amd.relu_dropout(h, p=0.5, seed=seed)
    assert len(out.grad_fn.saved_tensors) == 1 and out.grad_fn.saved_tensors[0].data_ptr() == out.data_ptr()
    out.sum().backward()
    devis_amd.relu_dropout(h.detach(), p=0.5, seed=seed)
    assert calls == ["relu_forward", "relu_backward", "relu_forward"]


# ---- the patch -------------------------------------------------------------------------------------------------------------------

def methods_of(module):
    return [module.DeformableTransformerEncoderLayer.__dict__.get(n) for n in ("forward", "forward_ffn")] + \
        [module.DeformableTransformerDecoderLayer.__dict__.get(n) for n in ("forward", "forward_ffn")]


def test_patch_sets_and_restores_and_leaves_the_other_patches_alone_in_both_orders():
    import devis_amd
    from devis_amd import argument_builders as AB
    from devis_amd.modules import transformer_layers as TL
    ours = [TL.encoder_forward, TL.encoder_forward_ffn, TL.decoder_forward, TL.decoder_forward_ffn]
    for transformer_first in (True, False):
        module = L.reference_module()
        theirs = methods_of(module)
        subclass = type("DeVISTransformerEncoderLayer", (module.DeformableTransformerEncoderLayer,), {})
        other = (module.DeformableTransformerEncoder.__dict__["get_reference_points"], module.DeformableTransformer.__dict__["prepare_data"])
        if transformer_first:
            undo_t = devis_amd.patch_transformer(module)
        undo = devis_amd.patch_transformer_layers(module)
        assert methods_of(module) == ours and subclass.forward is TL.encoder_forward          # the subclasses inherit
        assert sorted(undo.values(), key=id) == sorted(theirs, key=id)
        if not transformer_first:
            undo_t = devis_amd.patch_transformer(module)
        assert methods_of(module) == ours
        assert module.DeformableTransformerEncoder.get_reference_points is AB.get_reference_points
        assert module.DeformableTransformer.prepare_data is AB.prepare_data
        again = devis_amd.patch_transformer_layers(module)                                   # twice: the stock ones are remembered
        assert again == undo and methods_of(module) == ours
        if transformer_first:
            devis_amd.unpatch_transformer_layers(module, undo)
            assert module.DeformableTransformerEncoder.get_reference_points is AB.get_reference_points
            AB.unpatch_transformer(module, undo_t)
        else:
            AB.unpatch_transformer(module, undo_t)
            assert methods_of(module) == ours
            devis_amd.unpatch_transformer_layers(module, undo)
        assert methods_of(module) == theirs and subclass.forward is theirs[0]
        assert TL.STOCK not in module.DeformableTransformerEncoderLayer.__dict__
        assert (module.DeformableTransformerEncoder.__dict__["get_reference_points"], module.DeformableTransformer.__dict__["prepare_data"]) == other
    with pytest.raises(AttributeError):
        devis_amd.patch_transformer_layers(types.SimpleNamespace())
    assert "state dicts are untouched" in devis_amd.patch_transformer_layers.__doc__


@pytest.fixture()
def fused_on_cpu(monkeypatch):
    """The patched layers take the fused route on CPU tensors, the binding being the torch stand-in."""
    from devis_amd.modules import transformer_layers as TL
    calls = fake_addnorm.install(monkeypatch)
    monkeypatch.setattr(TL, "_on_gpu", lambda x: True)
    return calls


@pytest.mark.parametrize("kind", ["encoder", "decoder"])
def test_patched_stand_in_layers_reproduce_the_fixtures_and_take_effect_at_once(fused_on_cpu, monkeypatch, kind):
    import devis_amd
    calls = fused_on_cpu
    case, module = L.load_case(kind), L.reference_module()
    layer, inputs, attention = L.build_layer(module, kind, case)                 # a layer that exists before the patch
    keys = list(layer.state_dict())
    undo = devis_amd.patch_transformer_layers(module)
    try:
        out = layer(*inputs)
        sites = 2 if kind == "encoder" else 3
        assert calls == ["forward"] * (sites - 1) + ["relu_forward", "forward"]
        assert float((out.detach() - case["out"]).abs().max()) <= 1e-6 * float(case["out"].abs().max())
        check_case(L.run_case(module, kind, case), case, 1e-6, "patched " + kind)
        assert list(layer.state_dict()) == keys
        # forward_ffn on its own
        del calls[:]
        ffn = layer.forward_ffn(inputs[0])
        assert calls == ["relu_forward", "forward"] and ffn.shape == inputs[0].shape
        # training: one randint for the call's seeds, and dropout at every site
        layer.train()
        drawn = []
        real = torch.randint
        monkeypatch.setattr(torch, "randint", lambda *a, **k: drawn.append(a) or real(*a, **k))
        torch.manual_seed(5)
        a = layer(*inputs)
        assert len(drawn) == 1 and drawn[0][:3] == (-(1 << 63), (1 << 63) - 1, (sites + 1,))
        torch.manual_seed(5)
        b = layer(*inputs)
        torch.manual_seed(6)
        c = layer(*inputs)
        assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, out)
        layer.eval()
        # what sends a call to the replaced methods
        del calls[:]
        layer.activation = F.gelu
        layer(*inputs)
        layer.activation = F.relu
        assert calls == []
        plain = torch.nn.LayerNorm(L.D_MODEL, elementwise_affine=False).double()
        layer.norm1, kept = plain, layer.norm1
        layer(*inputs)
        layer.norm1 = kept
        assert calls == ["relu_forward", "forward"]          # (the replaced forward calls forward_ffn, which decides for itself)
    finally:
        devis_amd.unpatch_transformer_layers(module, undo)
    del calls[:]
    assert torch.equal(layer(*inputs), L.build_layer(module, kind, case)[0](*inputs)) and calls == []


def test_patched_layers_stay_on_the_replaced_methods_for_cpu_tensors(monkeypatch):
    import devis_amd
    calls = fake_addnorm.install(monkeypatch)
    case, module = L.load_case("encoder"), L.reference_module()
    layer, inputs, _ = L.build_layer(module, "encoder", case)
    want = layer(*inputs)
    undo = devis_amd.patch_transformer_layers(module)
    try:
        assert torch.equal(layer(*inputs), want) and calls == []
    finally:
        devis_amd.unpatch_transformer_layers(module, undo)


class _Anything(types.ModuleType):
    """A stand-in module: any attribute is a placeholder class (enough for `from x import Y`)."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF_SRC, "models", "deformable_transformer.py")),
                    reason="needs the reference tree (build container only)")
def test_patch_works_on_the_real_reference_classes(fused_on_cpu):
    """The reference's unmodified deformable_transformer.py, imported as tests/golden/make_golden_layerglue.py imports it (a
    package of its own name whose __init__ is skipped, stand-ins for the imports that are never called: with n_points=None the
    layers build no deformable attention): the patched real layers reproduce the fixtures recorded from them."""
    import importlib
    import devis_amd
    calls, name = fused_on_cpu, "layerglue_reference"
    try:
        for pkg, path in ((name, REF_SRC), (name + ".models", os.path.join(REF_SRC, "models")), (name + ".util", os.path.join(REF_SRC, "util"))):
            sys.modules[pkg] = types.ModuleType(pkg)
            sys.modules[pkg].__path__ = [path]
        for stub in (name + ".util.misc", name + ".models.ops", name + ".models.ops.modules"):
            sys.modules[stub] = _Anything(stub)
        module = importlib.import_module(name + ".models.deformable_transformer")
        assert module.__file__ == os.path.join(REF_SRC, "models", "deformable_transformer.py")
        theirs = methods_of(module)
        undo = devis_amd.patch_transformer_layers(module)
        try:
            for kind in ("encoder", "decoder"):
                case = L.load_case(kind)
                cls = module.DeformableTransformerEncoderLayer if kind == "encoder" else module.DeformableTransformerDecoderLayer
                build = lambda d, f, p, n_heads, cls=cls: cls(d_model=d, d_ffn=f, dropout=p, n_heads=n_heads, n_points=None)      # noqa: E731
                real = types.SimpleNamespace(DeformableTransformerEncoderLayer=build, DeformableTransformerDecoderLayer=build)
                del calls[:]
                check_case(L.run_case(real, kind, case), case, 1e-6, "real " + kind)
                assert calls.count("forward") == (2 if kind == "encoder" else 3) and calls.count("relu_forward") == 1
        finally:
            devis_amd.unpatch_transformer_layers(module, undo)
        assert methods_of(module) == theirs and None not in theirs
    finally:
        for key in [k for k in sys.modules if k == name or k.startswith(name + ".")]:
            del sys.modules[key]


# ---- the compiled path -----------------------------------------------------------------------------------------------------------

class Attention(torch.nn.Module):
    def forward(self, query, *args, **kwargs):
        return 0.5 * query, None


def test_compile_fullgraph_traces_the_replaced_chain(fused_on_cpu):
    import devis_amd
    calls = fused_on_cpu
    module = L.reference_module()
    torch.manual_seed(0)
    layer = module.DeformableTransformerEncoderLayer().eval()
    layer.self_attn = Attention()
    src, pos = torch.randn(2, 7, L.D_MODEL), torch.randn(2, 7, L.D_MODEL)
    want = layer(src, pos, None, None, None)
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    undo = devis_amd.patch_transformer_layers(module)
    try:
        eager = layer(src, pos, None, None, None)
        assert calls.count("forward") == 2 and torch.allclose(eager, want, atol=1e-5)
        del calls[:]
        torch._dynamo.reset()
        got = torch.compile(layer, fullgraph=True, backend=backend)(src, pos, None, None, None)
        assert torch.equal(got, want) and calls == [] and len(graphs) == 1
        targets = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function"]
        assert sum("layer_norm" in t for t in targets) == 2 and any("relu" in t for t in targets)
        # the public functions are the composite while compiling
        f = torch.compile(lambda x, d, w, b: devis_amd.add_layer_norm(x, d, w, b) + devis_amd.relu_dropout(x), fullgraph=True, backend=backend)
        w, b = torch.randn(L.D_MODEL), torch.randn(L.D_MODEL)
        assert torch.allclose(f(src, pos, w, b), F.layer_norm(src + pos, (L.D_MODEL,), w, b) + F.relu(src), atol=1e-6) and calls == []
    finally:
        devis_amd.unpatch_transformer_layers(module, undo)
        torch._dynamo.reset()


def test_the_namespace_has_no_new_op():
    import json
    import devis_amd  # noqa: F401
    from devis_amd import ops
    with open(os.path.join(ROOT, "tests", "golden", "op_schemas.json")) as f:
        want = json.load(f)
    prefix = ops.NAMESPACE + "::"
    names = sorted({n.split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith(prefix)})
    assert len(names) == len(want) == 34 and not any("norm" in n or "relu" in n for n in names)
    assert not hasattr(ops, "add_layer_norm") and "devis_amd.functions.add_norm" in sys.modules


# ---- documents ---------------------------------------------------------------------------------------------------------------

def test_the_documents_describe_the_operator():
    import devis_amd
    read = lambda name: open(os.path.join(ROOT, name)).read()      # noqa: E731
    design, integration, readme = read("DESIGN.md"), read("INTEGRATION.md"), read("README.md")
    assert re.search(r"^## 19\. .*LayerNorm", design, re.M)
    section = design.split("## 19.")[1]
    for phrase in ("Philox4x32-10", "torch.library", "launches", "scratch", "src + pos"):
        assert phrase in section, phrase
    assert re.search(r"^#+ Transformer layers: residual, dropout, LayerNorm", integration, re.M)
    assert "patch_transformer_layers" in integration.split("Transformer layers: residual, dropout, LayerNorm")[1]
    assert "add_layer_norm" in readme and "addnorm.h" in readme and "transformer_layers.py" in readme
    assert "addnorm.h" in devis_amd.__doc__ and "add_layer_norm" in devis_amd.__doc__
    assert os.path.exists(os.path.join(ROOT, "scripts", "addnorm_bench.py"))
    if not os.path.exists(os.path.join(ROOT, "profiles", "addnorm_bench.json")):
        assert "no ratio is quoted" in readme and "not measured" in readme
