"""CPU tests of the Swin glue (include/prenorm.h): the header against the binding, argument errors and the
workspace arithmetic without a GPU, the torch composite of both functions against the float64 oracle, the patched stage against
the fixture recorded from the reference, and -- on the test double tests/fake_prenorm.py -- which calls the patched blocks and
layers issue, which gradients the backward asks for, the fallbacks, the drop-path draws and the patch bookkeeping.

Tolerances.  Composite against oracle: 1e-10 of each tensor's maximum (both are float64).  Stage against the fixture: 1e-9
(tests/test_winattn_cpu.py's bar).  On the double the saved mean and rstd are float32, as the kernels keep them (relative
rounding 2^-24 = 6e-8 each, entering the gradients once or twice per norm and four norms deep): 1e-5 of each tensor's maximum."""
import ctypes
import os
import re

import pytest
import torch

import fake_prenorm
import fake_winattn
import prenorm_oracle as O
import swinglue_cases as S
from conftest import ROOT

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16


def close(got, want, tol, what):
    err, ref = float((got.detach().double() - want).abs().max()), float(want.abs().max())
    assert got.shape == want.shape and err <= tol * ref, (what, err, ref)


def check_fixture(got, case, tol, what):
    assert sorted(got) == sorted(k for k in case if k in ("x_out", "x_down") or k.startswith("grad.")), what
    for key in sorted(got):
        close(got[key], case[key], tol, "%s %s" % (what, key))


def rand(*shape, seed=0, dtype=F64):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64).to(dtype)


# ---- library -----------------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_prenorm_h_declares_and_versions_agree():
    from devis_amd import _prenorm, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "prenorm.h")).read()
    declared = set(re.findall(r"\b(prenorm_[a-z_0-9]+)\s*\(", header.split("#ifndef PRENORM_H")[1]))
    assert declared == set(_prenorm.EXPORTED_SYMBOLS) and len(declared) == 7
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _prenorm.load()
    assert lib.prenorm_version() == _prenorm.PRENORM_ABI_VERSION == int(re.search(r"#define PRENORM_ABI_VERSION (\d+)", header).group(1))
    assert int(re.search(r"#define PRENORM_MAX_CHANNELS (\d+)", header).group(1)) == _prenorm.MAX_CHANNELS == 3072
    assert lib.prenorm_tile(_prenorm.TILE_CHANNELS) == 3072 and _prenorm.tile() == lib.prenorm_tile(0) >= 1 and lib.prenorm_tile(7) == -1
    assert dict(re.findall(r"PRENORM_(F32|BF16|F16) = (\d)", header)) == {"F32": "0", "BF16": "2", "F16": "3"}
    assert dict(re.findall(r"PRENORM_(PLAIN|RESIDUAL|MERGE|TOKENS|MAP) = (\d)", header)) == {
        "PLAIN": str(_prenorm.PLAIN), "RESIDUAL": str(_prenorm.RESIDUAL), "MERGE": str(_prenorm.MERGE),
        "TOKENS": str(_prenorm.TOKENS), "MAP": str(_prenorm.MAP)}
    assert ctypes.sizeof(_prenorm.Shape) == 40 and ctypes.sizeof(_prenorm.Types) == 16
    fields = re.search(r"typedef struct prenorm_shape \{(.*?)\}", header, re.S).group(1)
    assert re.findall(r"\b(B|H|W|C|Hp|Wp|source|dest)\b(?=[,;])", fields) == [n for n, _ in _prenorm.Shape._fields_]
    assert os.path.join(build.include_dir(), "prenorm.h") in build._headers()
    assert any(s.endswith("prenorm.hip") for s in build.sources())
    assert "prenorm.h" in open(os.path.join(ROOT, "setup.py")).read() and "prenorm.h" in build.include_dir.__doc__
    from devis_amd import _binding
    assert "_prenorm" in _binding.__doc__
    source = open(os.path.join(ROOT, "devis_amd", "csrc", "prenorm.hip")).read()
    assert re.findall(r'#include "([^"]+)"', source) == ["op_common.h", "prenorm.h"]
    assert "atomic" not in source.split("namespace prenorm")[1] and "__shared__" not in source


def test_prenorm_argument_errors_and_workspace_size_without_gpu():
    from devis_amd import _prenorm
    lib = _prenorm.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.prenorm_last_error
    RES, MERGE, MAP = _prenorm.RESIDUAL, _prenorm.MERGE, _prenorm.MAP
    shape = lambda B=2, H=6, W=9, C=16, Hp=0, Wp=0, source=0, dest=0: ctypes.byref(_prenorm.Shape(B, H, W, C, Hp, Wp, source, dest))      # noqa: E731
    types = lambda x=0, delta=0, y=0, param=0: ctypes.byref(_prenorm.Types(x, delta, y, param))      # noqa: E731
    fwd = lambda t=types(), x=p, delta=None, keep=None, w=p, b=p, eps=1e-5, s=shape(), so=None, y=p, mean=None, rstd=None: \
        lib.prenorm_forward(t, x, delta, keep, w, b, eps, s, so, y, mean, rstd, None)      # noqa: E731
    bwd = lambda t=types(), x=p, keep=None, w=p, mean=p, rstd=p, gy=p, gs=None, s=shape(), wsp=p, gx=p, gd=None, gw=None, gb=None: \
        lib.prenorm_backward(t, x, keep, w, mean, rstd, gy, gs, s, wsp, gx, gd, gw, gb, None)      # noqa: E731
    size = lambda s: lib.prenorm_workspace_bytes(s)      # noqa: E731
    for call in (fwd, bwd, lambda s=shape(), **k: size(s), lambda s=shape(), **k: lib.prenorm_rows(s)):
        assert call(s=None) == -1 and b"null pointer" in err()
        assert call(s=shape(C=0)) == -1 and b"positive" in err()
        assert call(s=shape(C=3073)) == -1 and b"3072" in err()
        assert call(s=shape(C=18, source=MERGE)) == -1 and b"multiple of 4" in err()
        assert call(s=shape(Hp=5, Wp=12, dest=MAP)) == -1 and b"smaller" in err()
        assert call(s=shape(Hp=8, Wp=8, dest=MAP)) == -1 and b"smaller" in err()
        assert call(s=shape(Hp=8, Wp=12, source=MERGE, dest=MAP)) == -1 and b"no map" in err()
        assert call(s=shape(B=-1)) == -1 and b"negative" in err()
        assert call(s=shape(source=3)) == -1 and b"source" in err() and call(s=shape(dest=2)) == -1 and b"destination" in err()
        assert call(s=shape(B=1 << 20, H=1 << 10, W=1 << 10)) == -1 and b"31 bits" in err()
    for call in (fwd, bwd):
        # bad dtype mixes: float64; a code out of range; 16-bit x beside float32 delta or y; two 16-bit dtypes; 16-bit parameters
        # beside float32 x; a delta dtype without a delta
        for bad in (dict(x=1, delta=1, y=1, param=1), dict(x=9), dict(x=2, delta=0, y=2), dict(x=2, delta=2, y=0),
                    dict(x=0, delta=2, y=3), dict(x=0, delta=0, y=0, param=2), dict(x=2, delta=3, y=2, param=0)):
            assert call(t=types(**bad), s=shape(source=RES)) == -1 and b"dtype" in err(), bad
        assert call(t=types(delta=2)) == -1 and b"types.delta" in err()
        assert call(t=None) == -1 and b"null pointer" in err()
        for good in (dict(), dict(x=2, delta=2, y=2, param=2), dict(x=3, delta=3, y=3, param=0), dict(delta=2), dict(y=3),
                     dict(delta=2, y=2)):
            assert call(t=types(**good), s=shape(B=0, source=RES)) in (0, -1) and b"dtype" not in err(), good
    assert fwd(y=None) == -1 and b"null pointer" in err()
    assert fwd(x=None) == -1 and fwd(w=None) == -1 and fwd(b=None) == -1 and b"null pointer" in err()
    assert fwd(mean=p) == -1 and b"together" in err()
    assert fwd(delta=p) == -1 and fwd(so=p) == -1 and fwd(keep=p) == -1 and b"residual form" in err()
    assert fwd(s=shape(source=RES)) == -1 and fwd(s=shape(source=RES), delta=p) == -1 and b"null pointer" in err()
    assert fwd(eps=float("nan")) == -1 and b"eps" in err()
    assert bwd(gx=None) == -1 and b"no gradient" in err()                                       # every output NULL
    assert bwd(gd=p) == -1 and bwd(gs=p) == -1 and bwd(keep=p) == -1 and b"residual form" in err()
    for name in ("x", "mean", "rstd", "gy"):
        assert bwd(**{name: None}) == -1 and b"null pointer" in err(), name
    assert bwd(w=None) == -1 and b"weight" in err()
    assert bwd(s=shape(H=6, W=9), gw=p, wsp=None) == -1 and b"workspace" in err()                # 108 rows: four chunks
    assert bwd(gw=p, wsp=ctypes.c_void_p(p.value + 4)) == -1 and b"16-byte" in err()
    # nothing to compute: nothing is launched, nothing is dereferenced
    for empty in (shape(B=0), shape(H=0), shape(W=0), shape(B=0, Hp=8, Wp=12, dest=MAP)):
        assert fwd(s=empty, x=None, w=None, b=None) == 0
        assert bwd(s=empty, x=None, w=None, mean=None, rstd=None, gy=None, wsp=None) == 0
    # rows and the workspace: chunks of prenorm_tile() rows; chunks * 2 * C floats, rounded up to 256 bytes, 0 for one chunk
    tile = _prenorm.tile()
    for B, H, W, C, source in ((2, 6, 9, 16, 0), (1, 1, tile, 3072, 0), (1, 1, tile + 1, 260, RES), (2, 7, 9, 64, MERGE),
                               (6, 200, 334, 192, RES), (6, 200, 334, 768, MERGE), (1, 1, 1, 4, MERGE)):
        rows = B * ((H + 1) // 2) * ((W + 1) // 2) if source == MERGE else B * H * W
        chunks = -(-rows // tile)
        want = -(-(chunks * 2 * C * 4) // 256) * 256 if chunks > 1 else 0
        s = shape(B=B, H=H, W=W, C=C, source=source)
        assert lib.prenorm_rows(s) == rows and size(s) == want, (B, H, W, C, source)
        assert _prenorm.workspace_bytes(_prenorm.Shape(B, H, W, C, 0, 0, source, 0)) == want
    with pytest.raises(RuntimeError, match="3072"):
        _prenorm.workspace_bytes(_prenorm.Shape(1, 1, 1, 4000, 0, 0, 0, 0))


# ---- the composite route -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("map_size", [None, (6, 9, 8, 12)])
@pytest.mark.parametrize("residual,keep", [(False, None), (True, None), (True, [0.0, 1 / 0.7, 1 / 0.7])])
def test_residual_layer_norm_composite_equals_the_oracle_in_float64(residual, map_size, keep):
    import devis_amd
    B, L, C = 3, 54, 20
    x, delta, w, b = rand(B, L, C, seed=1), rand(B, L, C, seed=2), rand(C, seed=3) + 1, rand(C, seed=4)
    keep = None if keep is None else torch.tensor(keep, dtype=F64)
    gy, gs = rand(*((B, 8, 12, C) if map_size else (B, L, C)), seed=5), rand(B, L, C, seed=6)
    d = delta if residual else None
    want = O.forward(x, d, w, b, 1e-5, keep, None, map_size)
    want.update(O.grads(x, d, w, b, 1e-5, gy, gs if residual else None, keep, None, map_size))
    leaves = [t.clone().requires_grad_(True) for t in ((x, delta, w, b) if residual else (x, w, b))]
    s, y = devis_amd.residual_layer_norm(leaves[0], leaves[1] if residual else None, leaves[-2], leaves[-1], keep=keep, map_size=map_size)
    assert (s is leaves[0]) == (not residual)
    close(y, want["y"].view(y.shape), 1e-10, "y")
    if map_size:
        pad = y.detach().clone()
        pad[:, :6, :9] = 0
        assert not pad.any()
    grads = torch.autograd.grad([y, s], leaves, [gy, gs]) if residual else torch.autograd.grad(y, leaves, gy)
    names = ("grad_x", "grad_delta", "grad_weight", "grad_bias") if residual else ("grad_x", "grad_weight", "grad_bias")
    if residual:
        close(s, want["s"], 1e-10, "s")
    for name, g in zip(names, grads):
        close(g, want[name], 1e-10, name)


@pytest.mark.parametrize("H,W,C", [(5, 7, 16), (6, 9, 16), (4, 4, 4), (1, 1, 4), (3, 3, 6)])
def test_patch_merge_norm_composite_equals_the_oracle_in_float64(H, W, C):
    import devis_amd
    B = 2
    x, w, b = rand(B, H * W, C, seed=1), rand(4 * C, seed=2) + 1, rand(4 * C, seed=3)
    gy = rand(B, ((H + 1) // 2) * ((W + 1) // 2), 4 * C, seed=4)
    want = O.forward(x, None, w, b, 1e-5, merge=(H, W))
    want.update(O.grads(x, None, w, b, 1e-5, gy, merge=(H, W)))
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    y = devis_amd.patch_merge_norm(leaves[0], H, W, leaves[1], leaves[2])
    close(y, want["y"].view(y.shape), 1e-10, "y")
    for name, g in zip(("grad_x", "grad_weight", "grad_bias"), torch.autograd.grad(y, leaves, gy)):
        close(g, want[name], 1e-10, name)


def test_oracle_float32_order_is_a_sum_and_depends_on_C_alone():
    z = rand(5, 260, seed=9, dtype=F32).numpy()
    assert abs(O.row_sum_f32(z) - z.astype("float64").sum(1)).max() <= 1e-4
    wide = O.row_sum_f32(__import__("numpy").concatenate([z, 0 * z, 0 * z], 1))       # more (zero) groups: the same bits
    assert (wide == O.row_sum_f32(z)).all() and (O.var_f32(z) > 0).all()


def test_patched_stage_on_the_cpu_takes_the_composite_route_and_reproduces_the_fixture():
    import devis_amd
    from devis_amd.modules import swin_glue as G
    case = S.load_fixture()
    layer, x = S.build_layer(case)
    keys = list(layer.state_dict())
    stock = {name: getattr(S, name).forward for name in G.CLASSES}
    check_fixture(S.run_layer(layer, x, case), case, 1e-9, "stand-in stage")
    previous = devis_amd.patch_swin_glue(S)
    try:
        assert previous == stock and all(getattr(S, name).forward is G.FORWARDS[name] for name in G.CLASSES)
        assert list(layer.state_dict()) == keys
        check_fixture(S.run_layer(layer, x, case), case, 1e-9, "patched stage")
        assert devis_amd.patch_swin_glue(S) == previous      # twice: the recorded forwards stay
    finally:
        devis_amd.unpatch_swin_glue(S, previous)
    assert all(getattr(S, name).forward is stock[name] and G.PREVIOUS not in getattr(S, name).__dict__ for name in G.CLASSES)


# ---- on the test double --------------------------------------------------------------------------------------------------------

PLAIN, RES, MERGE, TOKENS, MAP = 0, 1, 2, 0, 1


def install(monkeypatch):
    calls = []
    fake_winattn.install(monkeypatch, calls)
    fake_prenorm.install(monkeypatch, calls)
    return calls


def forwards(calls):
    return [c for c in calls if c[0] == "forward" or c == "forward"]


@pytest.mark.parametrize("use_checkpoint", [False, True])
def test_patched_stage_issues_the_expected_calls_and_reproduces_the_fixture(monkeypatch, use_checkpoint):
    import devis_amd
    calls = install(monkeypatch)
    case = S.load_fixture()
    layer, x = S.build_layer(case, use_checkpoint=use_checkpoint)
    layer.train(use_checkpoint)                              # (every drop rate is 0, and the blocks' drop_path is nn.Identity)
    previous = devis_amd.patch_swin_glue(S)
    masks = S.BasicLayer.built_masks
    try:
        got = S.run_layer(layer, x, case)
    finally:
        devis_amd.unpatch_swin_glue(S, previous)
    assert S.BasicLayer.built_masks == masks                 # no mask construction
    check_fixture(got, case, 1e-5, "fused stage")
    first = [c for c in calls if c == "forward" or c[0] == "forward"][:7]
    block = [("forward", PLAIN, MAP, False), "forward", ("forward", RES, TOKENS, False)]
    chained = [("forward", RES, MAP, False), "forward", ("forward", RES, TOKENS, False)]
    # two calls per block around the attention's; the chained form after the first block; then the patch merging
    assert first == block + (block if use_checkpoint else chained) + [("forward", MERGE, TOKENS, False)]
    backwards = [c for c in calls if c[0] == "backward" and len(c) == 8]
    assert len(backwards) == 5 and backwards[0][:3] == ("backward", MERGE, TOKENS)
    assert all(c[3] and c[5] and c[6] for c in backwards)    # grad_x, grad_weight and grad_bias everywhere
    # grad_delta is never a tensor of its own without keep; s's gradient reaches the chained call
    assert not any(c[4] for c in backwards)
    plain = (PLAIN, MAP) if use_checkpoint else (RES, MAP)
    assert [c[1:3] for c in backwards] == [(MERGE, TOKENS), (RES, TOKENS), plain, (RES, TOKENS), (PLAIN, MAP)]
    assert [c[7] for c in backwards] == [False, True, not use_checkpoint, True, False]


def test_backward_asks_only_for_needed_gradients_and_shares_grad_delta(monkeypatch):
    import devis_amd
    calls = install(monkeypatch)
    B, L, C = 3, 12, 8
    x, delta, w, b = rand(B, L, C, seed=1), rand(B, L, C, seed=2), rand(C, seed=3) + 1, rand(C, seed=4)
    gy, gs = rand(B, L, C, seed=5), rand(B, L, C, seed=6)

    def run(needs, keep=None, use=("s", "y")):
        del calls[:]
        leaves = [t.clone().requires_grad_(n) for t, n in zip((x, delta, w, b), needs)]
        s, y = devis_amd.residual_layer_norm(*leaves, keep=keep)
        outs = [(s, gs)] * ("s" in use) + [(y, gy)] * ("y" in use)
        wanted = [t for t in leaves if t.requires_grad]
        grads = list(torch.autograd.grad([o for o, _ in outs], wanted, [g for _, g in outs], allow_unused=True))
        return [grads.pop(0) if n else None for n in needs], [c for c in calls if c[0] == "backward"]

    grads, back = run((True, True, True, True))
    assert back == [("backward", RES, TOKENS, True, False, True, True, True)]
    assert grads[1] is grads[0] or grads[1].data_ptr() == grads[0].data_ptr()        # grad_delta IS grad_x: one tensor, one store
    want = O.grads(x, delta, w, b, 1e-5, gy, gs)
    for name, g in zip(("grad_x", "grad_delta", "grad_weight", "grad_bias"), grads):
        close(g, want[name], 1e-5, name)
    keep = torch.tensor([0.0, 2.0, 2.0], dtype=F64)
    grads, back = run((True, True, False, False), keep)
    assert back == [("backward", RES, TOKENS, True, True, False, False, True)] and grads[1].data_ptr() != grads[0].data_ptr()
    want = O.grads(x, delta, w, b, 1e-5, gy, gs, keep)
    close(grads[0], want["grad_x"], 1e-5, "grad_x") or close(grads[1], want["grad_delta"], 1e-5, "grad_delta")
    assert not grads[1][0].any()
    assert run((False, True, False, False))[1] == [("backward", RES, TOKENS, True, False, False, False, True)]          # shared
    assert run((False, False, True, False))[1] == [("backward", RES, TOKENS, False, False, True, False, True)]
    assert run((False, False, False, True), use=("y",))[1] == [("backward", RES, TOKENS, False, False, False, True, False)]
    # an unused y costs nothing: s's gradient passes through by torch, no kernel
    grads, back = run((True, True, True, True), keep, use=("s",))
    assert back == [] and torch.equal(grads[0], gs) and torch.equal(grads[1], gs * keep.view(3, 1, 1)) and grads[2] is None
    # the patch merging: only what is asked for
    del calls[:]
    xm, wm, bm = rand(2, 35, 4, seed=7).requires_grad_(True), (rand(16, seed=8) + 1).requires_grad_(True), rand(16, seed=9)
    y = devis_amd.patch_merge_norm(xm, 5, 7, wm, bm)
    torch.autograd.grad(y, [xm, wm], rand(2, 12, 16, seed=10))
    assert calls == [("forward", MERGE, TOKENS, False), ("backward", MERGE, TOKENS, True, False, True, False, False)]
    # without autograd: no statistics, no Function
    del calls[:]
    with torch.no_grad():
        s, y = devis_amd.residual_layer_norm(x, delta, w, b)
    assert calls == [("forward", RES, TOKENS, False)] and not y.requires_grad
    close(y, O.forward(x, delta, w, b, 1e-5)["y"].view(y.shape), 1e-10, "y without autograd")


def test_each_fallback_condition_reaches_the_replaced_forward(monkeypatch):
    import devis_amd
    from devis_amd import _prenorm
    from devis_amd.functions import pre_norm as P
    from devis_amd.modules import swin_glue as G
    from devis_amd.modules import window_attention as M
    calls = install(monkeypatch)
    case = S.load_fixture()
    layer, x = S.build_layer(case)
    B, H, W = S.LAYER_INPUT
    with torch.no_grad():
        want = layer(x, H, W)
    previous = devis_amd.patch_swin_glue(S)
    ran = []
    for name in ("SwinTransformerBlock", "BasicLayer"):
        was = getattr(getattr(S, name), G.PREVIOUS)
        monkeypatch.setattr(getattr(S, name), G.PREVIOUS, lambda *a, was=was, name=name: ran.append(name) or was(*a))

    def run(expect_calls, expect_ran):
        del calls[:], ran[:]
        with torch.no_grad():
            got = layer(x, H, W)
        close(got[0], want[0], 1e-6, "x_out") or close(got[3], want[3], 1e-6, "x_down")
        assert bool(calls) == expect_calls and ran == expect_ran, (calls, ran)

    try:
        run(True, [])
        # a block that is not fusable: the whole layer runs the forward it replaced, and so does each block
        monkeypatch.setattr(M, "_on_gpu", lambda t: False)
        monkeypatch.setattr(P, "_on_gpu", lambda t: False)
        run(False, ["BasicLayer", "SwinTransformerBlock", "SwinTransformerBlock"])
        monkeypatch.setattr(M, "_on_gpu", lambda t: True)
        monkeypatch.setattr(P, "_on_gpu", lambda t: True)
        layer.blocks[1].norm2 = torch.nn.LayerNorm(16, elementwise_affine=False).double()
        try:
            del calls[:], ran[:]
            with torch.no_grad():
                layer(x, H, W)
            # (block 0 stays fusable when called alone: it takes the fused route from the replaced layer forward)
            assert ran == ["BasicLayer", "SwinTransformerBlock"] and ("forward", PLAIN, MAP, False) in calls
        finally:
            layer.blocks[1].norm2 = torch.nn.LayerNorm(16).double()
            layer.load_state_dict({k[len("state."):]: v for k, v in case.items() if k.startswith("state.")})
        # C above the limit
        monkeypatch.setattr(_prenorm, "MAX_CHANNELS", 8)
        run(False, ["BasicLayer", "SwinTransformerBlock", "SwinTransformerBlock"])
        monkeypatch.setattr(_prenorm, "MAX_CHANNELS", 3072)
        # while compiling
        monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
        run(False, ["BasicLayer", "SwinTransformerBlock", "SwinTransformerBlock"])
        monkeypatch.setattr(torch.compiler, "is_compiling", lambda: False)
        run(True, [])
    finally:
        devis_amd.unpatch_swin_glue(S, previous)
    # the functions themselves: the composite above the limit, in an unsupported mix and while compiling
    del calls[:]
    wide = rand(1, 2, 3076, seed=1)
    devis_amd.residual_layer_norm(wide, None, torch.ones(3076, dtype=F64), torch.zeros(3076, dtype=F64))
    devis_amd.residual_layer_norm(rand(1, 2, 8, dtype=BF16), rand(1, 2, 8, dtype=F32), torch.ones(8), torch.zeros(8))
    devis_amd.patch_merge_norm(rand(1, 4, 772, seed=1), 2, 2, torch.ones(3088, dtype=F64), torch.zeros(3088, dtype=F64))
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    devis_amd.residual_layer_norm(rand(1, 2, 8), None, torch.ones(8, dtype=F64), torch.zeros(8, dtype=F64))
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: False)
    assert calls == []


@pytest.mark.parametrize("fused", [False, True], ids=["composite route", "on the double"])
def test_drop_path_draws_are_the_stock_modules(monkeypatch, fused):
    """Training mode, drop_path = 0.3, the same torch.manual_seed: the patched stage and the stock stand-in stage agree."""
    import devis_amd
    if fused:
        calls = install(monkeypatch)
    layer, x = S.build_layer(drop_path=0.3)
    layer.train()
    B, H, W = S.LAYER_INPUT
    go, gd = rand(B, H * W, 16, seed=3), rand(B, 20, 32, seed=4)
    params = list(layer.parameters())

    def run(seed):
        torch.manual_seed(seed)
        out = layer(x, H, W)
        state = torch.get_rng_state()
        return [out[0].detach(), out[3].detach()] + list(torch.autograd.grad([out[0], out[3]], [x] + params, [go, gd])) + [state]

    seeds = (11, 12, 13, 14)                # (at 0.3 and B = 2, four seeds drop some entry in some block)
    want = [run(seed) for seed in seeds]
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(want, want[1:]))
    previous = devis_amd.patch_swin_glue(S)
    try:
        got = [run(seed) for seed in seeds]
    finally:
        devis_amd.unpatch_swin_glue(S, previous)
    for a, b in zip(got, want):
        assert torch.equal(a[-1], b[-1])                     # the generator was consumed as the stock forward consumes it
        for t, u in zip(a[:-1], b[:-1]):
            close(t, u, 1e-5 if fused else 1e-12, "drop path")
    if fused:
        assert ("forward", RES, TOKENS, True) in calls and ("forward", RES, MAP, True) in calls


def test_patching_and_unpatching_in_either_order_with_the_window_attention_patch_restores_the_forwards():
    import devis_amd
    from devis_amd.modules import swin_glue as G
    from devis_amd.modules import window_attention as M
    stock = {name: getattr(S, name).forward for name in G.CLASSES}

    def restored():
        return all(getattr(S, name).forward is stock[name] and G.PREVIOUS not in getattr(S, name).__dict__ for name in G.CLASSES) \
            and M.STOCK not in S.SwinTransformerBlock.__dict__

    # the window attention first
    a = devis_amd.patch_window_attention(S)
    b = devis_amd.patch_swin_glue(S)
    assert b["SwinTransformerBlock"] is M.block_forward and S.SwinTransformerBlock.forward is G.block_forward
    devis_amd.unpatch_swin_glue(S, b)
    assert S.SwinTransformerBlock.forward is M.block_forward and S.BasicLayer.forward is stock["BasicLayer"]
    devis_amd.unpatch_window_attention(S, a)
    assert restored()
    # the glue first
    b = devis_amd.patch_swin_glue(S)
    a = devis_amd.patch_window_attention(S)
    assert a["SwinTransformerBlock"] is G.block_forward and S.BasicLayer.forward is G.layer_forward
    devis_amd.unpatch_window_attention(S, a)
    assert S.SwinTransformerBlock.forward is G.block_forward
    devis_amd.unpatch_swin_glue(S, b)
    assert restored()
    # the window attention first, and undone first: its undoing has put the stock forward back, which stays
    a = devis_amd.patch_window_attention(S)
    b = devis_amd.patch_swin_glue(S)
    devis_amd.unpatch_window_attention(S, a)
    devis_amd.unpatch_swin_glue(S, b)
    assert restored()
    # alone
    b = devis_amd.patch_swin_glue(S)
    devis_amd.unpatch_swin_glue(S, b)
    assert restored()


# ---- documents ---------------------------------------------------------------------------------------------------------------

def test_the_documents_describe_the_operator():
    import devis_amd
    read = lambda name: open(os.path.join(ROOT, name)).read()      # noqa: E731
    design, integration, readme = read("DESIGN.md"), read("INTEGRATION.md"), read("README.md")
    assert re.search(r"^## 22\. .*Swin", design, re.M)
    section = design.split("## 22.")[1]
    for phrase in ("keep", "PRENORM_MAX_CHANNELS", "torch.library", "mean", "rstd", "chunks", "bitwise", "is_compiling", "GELU",
                   "PatchEmbed", "position embedding", "Attention dropout", "NCHW"):
        assert phrase in section, phrase
    assert re.search(r"^#+ Backbone: Swin block glue", integration, re.M)
    part = integration.split("Backbone: Swin block glue")[1]
    for phrase in ("patch_swin_glue", "mask_matrix", "use_checkpoint", "is_compiling", "drop_path", "float64"):
        assert phrase in part, phrase
    assert "residual_layer_norm" in readme and "prenorm.h" in readme and "swinglue_bench.py" in readme
    assert "prenorm.h" in devis_amd.__doc__ and "residual_layer_norm" in devis_amd.__doc__ and "patch_merge_norm" in devis_amd.__doc__
    assert os.path.exists(os.path.join(ROOT, "scripts", "swinglue_bench.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "prenorm_resource_usage.txt"))
