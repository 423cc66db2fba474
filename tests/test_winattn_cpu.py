"""CPU tests of the Swin backbone's window attention: the oracle (the mask rule against the sliced construction, the recorded
stage of the reference), the C ABI of include/winattn.h (exports, version, argument errors, the workspace size -- no compute
calls), the host code (checks, errors, which gradients are computed), the block's forward and the patch with the binding
replaced by the torch stand-in of tests/fake_winattn.py, the fallbacks and the compiled path.  The kernels themselves are
tests/test_winattn_gpu.py."""
import ctypes
import os
import re

import pytest
import torch

import fake_winattn
import winattn_cases as C
import winattn_oracle as O
from conftest import ROOT

F32, F64 = torch.float32, torch.float64
FIXTURE_TOL = 1e-9                      # of each tensor's maximum, in float64


def check_fixture(got, case, what):
    wanted = [k for k in case if k == "out" or k.startswith("grad.")]
    assert sorted(got) == sorted(wanted) and len(wanted) == 1 + 1 + 2 * 13, what            # out, grad.x, 13 parameters per block
    for key in sorted(got):
        want = case[key]
        err, ref = float((got[key].detach().double().cpu() - want).abs().max()), float(want.abs().max())
        print("%s %s: max error %.3e, max |want| %.3e" % (what, key, err, ref))
        assert ref > 0 and err <= FIXTURE_TOL * ref, (what, key, err, ref)


# ---- oracle ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ws,shift,Hp,Wp", [(7, 3, 14, 21), (7, 3, 7, 7), (7, 3, 7, 14), (12, 6, 12, 24), (4, 2, 8, 4), (5, 2, 10, 15),
                                            (4, 1, 4, 4)])
def test_region_rule_equals_the_sliced_mask(ws, shift, Hp, Wp):
    rule, sliced = O.shift_mask(Hp, Wp, ws, shift), O.sliced_mask(Hp, Wp, ws, shift)
    assert rule.shape == ((Hp // ws) * (Wp // ws), ws * ws, ws * ws) and torch.equal(rule, sliced)
    assert set(rule.unique().tolist()) <= {0.0, -100.0} and bool((rule == -100.0).any())
    assert O.shift_mask(Hp, Wp, ws, 0) is None


def test_relative_rows_are_the_headers_and_cover_the_table():
    for ws in (2, 4, 7):
        rows = O.relative_rows(ws)
        assert rows.min() == 0 and rows.max() == (2 * ws - 1) ** 2 - 1 and len(rows.unique()) == (2 * ws - 1) ** 2
        assert bool((rows.diagonal() == ((2 * ws - 1) ** 2 - 1) // 2).all())
        from devis_amd.functions import window_attention as A
        assert torch.equal(A.relative_rows(ws), rows)
        assert torch.equal(A.shift_regions(3 * ws, 2 * ws, ws, ws // 2), O.region_map(3 * ws, 2 * ws, ws, ws // 2))


def test_reference_shaped_stage_reproduces_the_fixture():
    """The stage of tests/winattn_cases.py -- the oracle's chain inside reference-shaped modules -- against what the reference's
    own BasicLayer recorded."""
    case = C.load_fixture()
    layer, x = C.build_layer(case)
    check_fixture(C.run_layer(layer, x, case), case, "oracle stage")
    assert [blk.shift_size for blk in layer.blocks] == [0, 2] and case["x"].shape == (2, 54, 16)
    for name in os.listdir(C.GOLDEN):
        if name.startswith("winattn_"):
            assert name.endswith(".py") or os.path.getsize(os.path.join(C.GOLDEN, name)) < 32 << 10, name


def test_oracle_equals_the_window_module_on_the_partitioned_map():
    ws, shift, Hp, Wp, B, H, D = C.SHAPES[2]
    qkv, table, go = C.make_inputs(C.SHAPES[2], F64)
    want = O.attention(qkv, table, H, ws, shift)
    # by hand, for one output pixel: window (1, 2), token (3, 1) -> shifted (8, 11) -> map pixel (0, 13)
    wy, wx, iy, ix = 1, 2, 3, 1
    ys, xs = wy * ws + iy, wx * ws + ix
    y, x = (ys + shift) % Hp, (xs + shift) % Wp
    regions = O.region_map(Hp, Wp, ws, shift)
    C_ = H * D
    for h in range(H):
        q = qkv[1, y, x, h * D:(h + 1) * D]
        logits, values = [], []
        for jy in range(ws):
            for jx in range(ws):
                ky, kx = wy * ws + jy, wx * ws + jx
                py, px = (ky + shift) % Hp, (kx + shift) % Wp
                s = D ** -0.5 * float(q @ qkv[1, py, px, C_ + h * D:C_ + (h + 1) * D])
                s += float(table[(iy - jy + ws - 1) * (2 * ws - 1) + (ix - jx + ws - 1), h])
                s += -100.0 if regions[ys, xs] != regions[ky, kx] else 0.0
                logits.append(s)
                values.append(qkv[1, py, px, 2 * C_ + h * D:2 * C_ + (h + 1) * D])
        p = torch.softmax(torch.tensor(logits, dtype=F64), 0)
        by_hand = (p[:, None] * torch.stack(values)).sum(0)
        assert float((want[1, y, x, h * D:(h + 1) * D] - by_hand).abs().max()) <= 1e-12


# ---- library -----------------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_winattn_h_declares_and_versions_agree():
    from devis_amd import _native, _selfattn, _winattn, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "winattn.h")).read()
    declared = set(re.findall(r"\b(winattn_[a-z_0-9]+)\s*\(", header.split("#ifndef WINATTN_H")[1]))
    assert declared == set(_winattn.EXPORTED_SYMBOLS) and len(declared) == 5
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _winattn.load()
    assert lib.winattn_version() == _winattn.WINATTN_ABI_VERSION == 1 == int(re.search(r"#define WINATTN_ABI_VERSION (\d+)", header).group(1))
    assert dict(re.findall(r"WINATTN_(F32|F64|BF16|F16) = (\d)", header)) == {"F32": "0", "F64": "1", "BF16": "2", "F16": "3"}
    assert int(re.search(r"#define WINATTN_MAX_HEAD_DIM (\d+)", header).group(1)) == _winattn.MAX_HEAD_DIM == 64
    assert int(re.search(r"#define WINATTN_MAX_WINDOW (\d+)", header).group(1)) == _winattn.MAX_WINDOW >= 12
    assert ctypes.sizeof(_winattn.Shape) == 56
    assert _native.load().msda_build_info().decode() == "abi=14 arch=gfx950" and _selfattn.load().selfattn_version() == 2
    assert os.path.join(build.include_dir(), "winattn.h") in build._headers()
    assert any(s.endswith("winattn.hip") for s in build.sources())
    assert "winattn.h" in open(os.path.join(ROOT, "setup.py")).read() and "winattn.h" in build.include_dir.__doc__
    for phrase in ("(iy - jy + ws - 1) * (2 ws - 1) + (ix - jx + ws - 1)", "((ys + shift) mod Hp, (xs + shift) mod Wp)", "-100.0",
                   "region = 3 * r(ys, Hp) + r(xs, Wp)", "r(c, n) = (c >= n - ws) + (c >= n - shift)", "part * nH + h"):
        assert phrase in header, phrase
    # the unit shares no code with selfattn.hip
    source = open(os.path.join(ROOT, "devis_amd", "csrc", "winattn.hip")).read()
    assert re.findall(r'#include "([^"]+)"', source) == ["op_common.h", "winattn.h"] and "atomicAdd" not in source


def test_winattn_argument_errors_and_workspace_size_without_gpu():
    from devis_amd import _winattn
    lib = _winattn.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.winattn_last_error
    shape = lambda B=2, Hp=14, Wp=21, heads=2, head_dim=32, window=7, shift=3: ctypes.byref(      # noqa: E731
        _winattn.Shape(B, Hp, Wp, heads, head_dim, window, shift))
    fwd = lambda dt=0, wide=0, qkv=p, table=p, scale=0.5, s=shape(), out=p, lse=p, acc=None: lib.winattn_forward(      # noqa: E731
        dt, wide, qkv, table, scale, s, out, lse, acc, None)
    bwd = lambda dt=0, wide=0, qkv=p, table=p, out=p, go=p, lse=p, scale=0.5, s=shape(), gq=p, gt=p, wsp=p: lib.winattn_backward(      # noqa: E731
        dt, wide, qkv, table, out, go, lse, scale, s, gq, gt, wsp, None)
    size = lambda s: lib.winattn_workspace_bytes(s)      # noqa: E731
    for call in (fwd, bwd, lambda s=shape(), **k: size(s)):
        assert call(s=None) == -1 and b"null pointer" in err()
        assert call(s=shape(B=-1)) == -1 and b"negative" in err()
        assert call(s=shape(Hp=7 << 29)) == -1 and b"31 bits" in err()
        assert call(s=shape(B=1 << 20, Hp=7 << 10, Wp=7 << 10)) == -1 and b"31 bits" in err()
        assert call(s=shape(heads=0)) == -1 and b"heads" in err()
        for D in (6, 2, 68, 0):
            assert call(s=shape(head_dim=D)) == -1 and b"head dimension" in err(), D
        for ws in (0, 17):
            assert call(s=shape(window=ws, Hp=34, Wp=34, shift=0)) == -1 and b"window size" in err(), ws
        for shift in (-1, 7):
            assert call(s=shape(shift=shift)) == -1 and b"shift" in err(), shift
        assert call(s=shape(Hp=15)) == -1 and call(s=shape(Wp=20)) == -1 and b"multiples of the window" in err()
    for call in (fwd, bwd):
        assert call(dt=9) == -1 and b"dtype" in err()
        assert call(dt=1) == -1 and b"float64" in err()
        for bad in (float("nan"), float("inf")):
            assert call(scale=bad) == -1 and b"finite" in err()
        for name in ("qkv", "table"):
            assert call(**{name: None}) == -1 and b"null pointer" in err(), name
        assert call(s=shape(B=1 << 16, Hp=112, Wp=112, heads=32)) == -1 and b"too many workgroups" in err()
    assert fwd(out=None) == -1 and b"null pointer" in err()
    for name in ("out", "go", "lse"):
        assert bwd(**{name: None}) == -1 and b"null pointer" in err(), name
    assert bwd(wsp=None) == -1 and b"workspace" in err()
    # nothing to compute: nothing is launched, nothing is dereferenced
    nothing = dict(qkv=None, table=None, out=None, lse=None)
    for empty in (shape(B=0), shape(Hp=0), shape(Wp=0)):
        assert fwd(s=empty, **nothing) == 0
        assert bwd(s=empty, go=None, gq=None, gt=None, wsp=None, **nothing) == 0
        assert bwd(s=empty, go=None, wsp=None, **nothing) == 0
    assert bwd(gq=None, gt=None, go=None, wsp=None, **nothing) == 0                          # no gradient is asked for
    # the workspace: (chunks + 1) [nH, N, N] float planes; chunks = ceil(windows / ceil(windows / min(ceil(16384 / (QT^2 nH)), 256, windows)))
    def want(B, Hp, Wp, heads, ws):
        N = ws * ws
        QT, windows = -(-N // 16), B * (Hp // ws) * (Wp // ws)
        chunks = max(1, min(-(-16384 // (QT * QT * heads)), 256, windows))
        per = -(-windows // chunks)
        return (-(-windows // per) + 1) * heads * N * N * 4
    for B, Hp, Wp, heads, ws in ((2, 14, 21, 2, 7), (6, 203, 336, 6, 7), (1, 12, 24, 1, 12), (1, 4, 4, 1, 4), (6, 28, 42, 48, 7), (3, 4, 6, 2, 2)):
        assert size(shape(B=B, Hp=Hp, Wp=Wp, heads=heads, window=ws, shift=0)) == want(B, Hp, Wp, heads, ws), (B, Hp, Wp, heads, ws)
    assert size(shape(B=0)) == 2 * 2 * 49 * 49 * 4


def test_operator_raises_on_cpu_tensors_and_on_bad_arguments_before_any_launch(monkeypatch):
    import devis_amd
    from devis_amd import _winattn
    from devis_amd.functions import window_attention as A

    def no_launch(*a, **k):
        raise AssertionError("a kernel call was made")

    monkeypatch.setattr(_winattn, "forward", no_launch)
    monkeypatch.setattr(_winattn, "backward", no_launch)
    qkv, table = torch.zeros(1, 4, 4, 24), torch.zeros(49, 2)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.window_attention(qkv, table, 2, 4)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.window_attention(qkv.clone().requires_grad_(True), table, 2, 4, 2)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        A._backward(torch.zeros(1, 4, 4, 8), qkv, table, torch.zeros(1, 4, 4, 8), torch.zeros(1, 1, 2, 16), 2, 4, 0, None, (True, True))
    for name in ("window_attention", "patch_window_attention", "unpatch_window_attention"):
        assert name in devis_amd.__all__ and hasattr(devis_amd, name)
    assert devis_amd.window_attention is A.window_attention
    assert devis_amd.patch_window_attention is devis_amd.argument_builders.patch_window_attention
    assert "no CPU path" in A.__doc__ and "state dicts are untouched" in devis_amd.patch_window_attention.__doc__

    meta = lambda *s, dtype=F32: torch.zeros(*s, dtype=dtype, device="meta")      # noqa: E731
    bf, f16 = torch.bfloat16, torch.float16
    assert A.check_shapes(meta(2, 14, 21, 192), meta(169, 2), 2, 7, 3) == (2, 14, 21, 64, 2, 32, 7, 3, False)
    assert A.check_shapes(meta(0, 4, 4, 12, dtype=bf), meta(9, 1), 1, 2, 1) == (0, 4, 4, 4, 1, 4, 2, 1, True)
    for dtype, D, ws, ok in ((F32, 4, 2, True), (bf, 32, 7, True), (f16, 64, 12, True), (F32, 20, 16, True), (F64, 32, 7, False),
                             (F32, 68, 7, False), (F32, 6, 7, False), (F32, 32, 17, False), (F32, 32, 0, False), (torch.int32, 4, 4, False)):
        assert A.supported(dtype, D, ws) is ok, (dtype, D, ws)
    bad = [
        ("is required", lambda: A.check_shapes(meta(14, 21, 192), meta(169, 2), 2, 7, 3)),
        ("not divisible", lambda: A.check_shapes(meta(2, 14, 21, 190), meta(169, 2), 2, 7, 3)),
        ("head dimension", lambda: A.check_shapes(meta(2, 14, 21, 36), meta(169, 2), 2, 7, 3)),
        ("head dimension", lambda: A.check_shapes(meta(2, 14, 21, 3 * 136), meta(169, 2), 2, 7, 3)),
        ("window size", lambda: A.check_shapes(meta(2, 34, 34, 24), meta(33 * 33, 2), 2, 17, 0)),
        ("shift", lambda: A.check_shapes(meta(2, 14, 21, 24), meta(169, 2), 2, 7, 7)),
        ("shift", lambda: A.check_shapes(meta(2, 14, 21, 24), meta(169, 2), 2, 7, -1)),
        ("not a multiple of the window", lambda: A.check_shapes(meta(2, 15, 21, 24), meta(169, 2), 2, 7, 3)),
        ("bias_table must be", lambda: A.check_shapes(meta(2, 14, 21, 24), meta(168, 2), 2, 7, 3)),
        ("bias_table must be", lambda: A.check_shapes(meta(2, 14, 21, 24), meta(169, 3), 2, 7, 3)),
        ("unsupported dtype", lambda: A.check_shapes(meta(2, 14, 21, 24, dtype=F64), meta(169, 2, dtype=F64), 2, 7, 3)),
        ("bias_table must have the dtype", lambda: A.check_shapes(meta(2, 14, 21, 24), meta(169, 2, dtype=bf), 2, 7, 3)),
        ("bias_table must have the dtype", lambda: A.check_shapes(meta(2, 14, 21, 24, dtype=f16), meta(169, 2, dtype=bf), 2, 7, 3)),
        ("head dimension", lambda: devis_amd.window_attention(torch.zeros(1, 4, 4, 36), torch.zeros(49, 2), 2, 4)),
    ]
    for match, call in bad:
        with pytest.raises(RuntimeError, match=match):
            call()


# ---- the Function on the torch stand-in ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [C.SHAPES[1], C.SHAPES[2], C.UNSHIFTED[1]], ids=C.case_id)
def test_function_equals_the_oracle_in_float64(monkeypatch, case):
    import devis_amd
    fake_winattn.install(monkeypatch)
    ws, shift, Hp, Wp, B, H, D = case
    qkv, table, go = C.make_inputs(case, F64)
    want = O.attention_grads(qkv, table, H, ws, shift, go)
    a, b = qkv.clone().requires_grad_(True), table.clone().requires_grad_(True)
    out = devis_amd.window_attention(a, b, H, ws, shift)
    got = (out,) + torch.autograd.grad(out, (a, b), go)
    for x, y in zip(got, want):
        assert x.shape == y.shape and float((x - y).detach().abs().max()) <= 1e-12
    assert float((devis_amd.window_attention(qkv, table, H, ws, shift, scale=0.3) - O.attention(qkv, table, H, ws, shift, 0.3)).abs().max()) <= 1e-12
    with pytest.raises(RuntimeError, match="once_differentiable"):
        out = devis_amd.window_attention(a, b, H, ws, shift)
        g, = torch.autograd.grad((out * out).sum(), a, create_graph=True)
        g.sum().backward()


def test_function_computes_only_the_gradients_asked_for(monkeypatch):
    import devis_amd
    from devis_amd.functions import window_attention as A
    calls = fake_winattn.install(monkeypatch)
    case = C.SHAPES[2]
    ws, shift, Hp, Wp, B, H, D = case
    make = lambda: list(C.make_inputs(case, F32)[:2])      # noqa: E731
    ts = [t.requires_grad_(True) for t in make()]
    out = devis_amd.window_attention(*ts, H, ws, shift)
    full = torch.autograd.grad((out * out).sum(), ts)
    del calls[:]
    with torch.no_grad():
        devis_amd.window_attention(*ts, H, ws, shift)
    assert not devis_amd.window_attention(*make(), H, ws, shift).requires_grad and calls == ["forward", "forward"]
    for asked in ((0,), (1,), (0, 1)):
        ts = make()
        for i in asked:
            ts[i].requires_grad_(True)
        del calls[:]
        out = devis_amd.window_attention(*ts, H, ws, shift)
        grads = torch.autograd.grad((out * out).sum(), [ts[i] for i in asked])
        for i, g in zip(asked, grads):
            assert torch.equal(g, full[i]) and g.dtype == ts[i].dtype and g.is_contiguous() and g.shape == ts[i].shape, (asked, i)
        assert calls == ["forward", ("backward",) + tuple(i in asked for i in range(2))], (asked, calls)
    # the saved tensors: qkv, the table, out and lse -- no windows, no probabilities, no mask
    qkv, table = (t.requires_grad_(True) for t in make())
    out = A.WindowAttentionFunction.apply(qkv, table, H, ws, shift, None)[0]
    saved = out.grad_fn.saved_tensors
    C_ = H * D
    assert [tuple(t.shape) for t in saved] == [(B, Hp, Wp, 3 * C_), ((2 * ws - 1) ** 2, H), (B, Hp, Wp, C_), (B, (Hp // ws) * (Wp // ws), H, ws * ws)]
    assert saved[0].data_ptr() == qkv.data_ptr() and saved[2].data_ptr() == out.data_ptr() and saved[3].dtype == F32
    # 16-bit operands beside a float32 table: the backward takes out before its rounding, gradients in the operands' dtypes
    qkv, table, go = C.make_inputs(case, torch.bfloat16, F32)
    qkv.requires_grad_(True), table.requires_grad_(True)
    out, lse, acc = A.WindowAttentionFunction.apply(qkv, table, H, ws, shift, None)
    assert out.dtype == torch.bfloat16 and acc.dtype == F32 and torch.equal(acc.to(torch.bfloat16), out) and not acc.requires_grad
    assert out.grad_fn.saved_tensors[2].data_ptr() == acc.data_ptr()
    gq, gt = torch.autograd.grad(out, (qkv, table), go)
    assert gq.dtype == torch.bfloat16 and gt.dtype == F32
    # an empty batch: no launch
    del calls[:]
    empty = torch.zeros(0, Hp, Wp, 3 * C_, requires_grad=True)
    out = devis_amd.window_attention(empty, table.detach().requires_grad_(True), H, ws, shift)
    assert out.shape == (0, Hp, Wp, C_) and calls == []


# ---- the block and the patch ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_checkpoint", [False, True])
def test_patched_stage_reproduces_the_fixture(monkeypatch, use_checkpoint):
    import devis_amd
    from devis_amd.modules import window_attention as M
    calls = fake_winattn.install(monkeypatch)
    case = C.load_fixture()
    layer, x = C.build_layer(case, use_checkpoint=use_checkpoint)
    keys = list(layer.state_dict())
    stock = C.SwinTransformerBlock.forward
    previous = devis_amd.patch_window_attention(C)
    try:
        assert C.SwinTransformerBlock.forward is M.block_forward and list(layer.state_dict()) == keys
        layer.train(use_checkpoint)                          # (every drop rate is 0)
        check_fixture(C.run_layer(layer, x, case), case, "patched stage")
        forwards = 4 if use_checkpoint else 2                # (a checkpointed block runs its forward again in the backward)
        assert calls.count("forward") == forwards and calls.count(("backward", True, True)) == 2 and len(calls) == forwards + 2
        # mask_matrix is not read
        del calls[:]
        blk = layer.blocks[1]
        tokens = case["x"].double()
        with torch.no_grad():
            a, b = blk(tokens, None), blk(tokens, torch.full((6, 16, 16), float("nan"), dtype=F64))
        assert torch.equal(a, b) and calls == ["forward", "forward"]
        assert devis_amd.patch_window_attention(C) == previous          # twice: the stock forward is still the recorded one
    finally:
        devis_amd.unpatch_window_attention(C, previous)
    assert C.SwinTransformerBlock.forward is stock and M.STOCK not in C.SwinTransformerBlock.__dict__
    del calls[:]
    layer.eval()
    check_fixture(C.run_layer(layer, x, case), case, "unpatched stage")
    assert calls == [] and list(layer.state_dict()) == keys


def test_block_pads_only_when_needed_and_projects_the_unpadded_tokens(monkeypatch):
    import devis_amd
    import torch.nn.functional as F
    calls = fake_winattn.install(monkeypatch)
    torch.manual_seed(3)
    blk = C.SwinTransformerBlock(16, 2, window_size=4, shift_size=2).double().eval()
    previous = devis_amd.patch_window_attention(C)
    try:
        pads, projected = [], []
        real_pad = F.pad
        monkeypatch.setattr(F, "pad", lambda *a, **k: pads.append(a[1]) or real_pad(*a, **k))
        blk.attn.proj.register_forward_hook(lambda m, i, o: projected.append(tuple(i[0].shape)))
        blk.H, blk.W = 8, 12
        blk(torch.randn(2, 96, 16, dtype=F64), None)
        assert pads == [] and projected == [(2, 96, 16)]
        blk.H, blk.W = 6, 9
        blk(torch.randn(2, 54, 16, dtype=F64), None)
        assert pads == [(0, 0, 0, 3, 0, 2)] and projected[1] == (2, 54, 16) and calls == ["forward", "forward"]
    finally:
        devis_amd.unpatch_window_attention(C, previous)


def test_each_fallback_condition_reaches_the_stock_forward(monkeypatch):
    import devis_amd
    from devis_amd.functions import window_attention as A
    from devis_amd.modules import window_attention as M
    calls = fake_winattn.install(monkeypatch)
    torch.manual_seed(4)
    x = torch.randn(2, 54, 16, dtype=F64)

    def block(**kwargs):
        torch.manual_seed(5)
        blk = C.SwinTransformerBlock(16, 2, window_size=4, shift_size=2, **kwargs).double().eval()
        blk.H, blk.W = 6, 9
        return blk

    blk = block()
    mask = O.sliced_mask(8, 12, 4, 2)
    want = blk(x, mask)
    ran = []
    previous = devis_amd.patch_window_attention(C)
    stock = getattr(C.SwinTransformerBlock, M.STOCK)
    monkeypatch.setattr(C.SwinTransformerBlock, M.STOCK, lambda *a: ran.append(1) or stock(*a))

    def falls_back(b, *args):
        del calls[:], ran[:]
        out = b(*args)
        assert calls == [] and ran == [1], args
        return out

    try:
        del calls[:]
        assert float((blk(x, None) - want).detach().abs().max()) <= 1e-12 and calls == ["forward"] and ran == []
        # not on the GPU; compiling
        monkeypatch.setattr(M, "_on_gpu", lambda t: False)
        assert torch.equal(falls_back(blk, x, mask), want)
        monkeypatch.setattr(M, "_on_gpu", lambda t: True)
        monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
        assert torch.equal(falls_back(blk, x, mask), want)
        monkeypatch.setattr(torch.compiler, "is_compiling", lambda: False)
        # float64 (the double takes it; the kernels do not)
        monkeypatch.setattr(A, "DTYPES", (F32, torch.bfloat16, torch.float16))
        assert torch.equal(falls_back(blk, x, mask), want)
        monkeypatch.setattr(A, "DTYPES", (F32, torch.bfloat16, torch.float16, F64))
        # attention dropout: in training only
        dropping = block(attn_drop=0.5)
        del calls[:]
        dropping(x, mask)
        assert calls == ["forward"]
        dropping.train()
        falls_back(dropping, x, mask)
        # a head dimension or a window the kernels do not take
        odd = C.SwinTransformerBlock(12, 2, window_size=4, shift_size=0).double().eval()         # D = 6
        odd.H, odd.W = 4, 4
        falls_back(odd, torch.randn(1, 16, 12, dtype=F64), None)
        monkeypatch.setattr(devis_amd._winattn, "MAX_WINDOW", 3)
        assert torch.equal(falls_back(blk, x, mask), want)
        monkeypatch.setattr(devis_amd._winattn, "MAX_WINDOW", 16)
        # not [B, L, C]
        with pytest.raises(Exception):
            falls_back(blk, x[0], mask)
    finally:
        devis_amd.unpatch_window_attention(C, previous)


# ---- the compiled path -----------------------------------------------------------------------------------------------------------

def test_composite_equals_the_oracle_with_gradients():
    from devis_amd.functions import window_attention as A
    for case in (C.SHAPES[1], C.SHAPES[2], C.UNSHIFTED[0]):
        ws, shift, Hp, Wp, B, H, D = case
        qkv, table, go = C.make_inputs(case, F64)
        want = O.attention_grads(qkv, table, H, ws, shift, go)
        a, b = qkv.clone().requires_grad_(True), table.clone().requires_grad_(True)
        out = A.composite(a, b, H, ws, shift)
        for x, y in zip((out,) + torch.autograd.grad(out, (a, b), go), want):
            assert float((x - y).detach().abs().max()) <= 1e-12


def test_compile_fullgraph_traces_the_composite_and_the_stock_block(monkeypatch):
    import devis_amd
    calls = fake_winattn.install(monkeypatch)
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    ws, shift, Hp, Wp, B, H, D = C.SHAPES[1]
    qkv, table, _ = C.make_inputs(C.SHAPES[1], F32)
    previous = devis_amd.patch_window_attention(C)
    try:
        torch._dynamo.reset()
        f = torch.compile(lambda a, b: devis_amd.window_attention(a, b, H, ws, shift), fullgraph=True, backend=backend)
        assert float((f(qkv, table).double() - O.attention(qkv.double(), table.double(), H, ws, shift)).abs().max()) <= 1e-5
        torch.manual_seed(6)
        blk = C.SwinTransformerBlock(16, 2, window_size=4, shift_size=2).eval()
        blk.H, blk.W = 6, 9
        x, mask = torch.randn(2, 54, 16), O.sliced_mask(8, 12, 4, 2).float()
        got = torch.compile(blk, fullgraph=True, backend=backend)(x, mask)
        assert calls == [] and len(graphs) == 2
        devis_amd.unpatch_window_attention(C, previous)
        previous = None
        assert torch.allclose(got, blk(x, mask), atol=1e-6)
    finally:
        if previous is not None:
            devis_amd.unpatch_window_attention(C, previous)
        torch._dynamo.reset()


# ---- documents ---------------------------------------------------------------------------------------------------------------

def test_the_documents_describe_the_operator():
    import devis_amd
    read = lambda name: open(os.path.join(ROOT, name)).read()      # noqa: E731
    design, integration, readme = read("DESIGN.md"), read("INTEGRATION.md"), read("README.md")
    assert re.search(r"^## 21\. .*window attention", design, re.M)
    section = design.split("## 21.")[1]
    for phrase in ("mask_matrix", "not read", "torch.library", "lse", "-100", "region", "chunks", "bitwise", "is_compiling", "1e-4"):
        assert phrase in section, phrase
    assert re.search(r"^#+ Backbone: Swin window attention", integration, re.M)
    part = integration.split("Backbone: Swin window attention")[1]
    for phrase in ("patch_window_attention", "mask_matrix", "use_checkpoint", "is_compiling", "attn_drop", "float64", "Not implemented on the CPU"):
        assert phrase in part, phrase
    assert "window_attention" in readme and "winattn.h" in readme and "winattn_bench.py" in readme
    assert "winattn.h" in devis_amd.__doc__ and "window_attention" in devis_amd.__doc__
    assert os.path.exists(os.path.join(ROOT, "scripts", "winattn_bench.py"))
    if not os.path.exists(os.path.join(ROOT, "profiles", "winattn_bench.json")):
        assert "not recorded" in readme
