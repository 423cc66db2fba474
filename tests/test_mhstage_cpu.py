"""CPU tests of the mask-head stage: the oracle against the reference fixtures, the C ABI of include/mhstage.h (exports,
version, argument errors, workspace arithmetic -- no compute calls), the host code (shape checks, errors, gradient masks, the
index rule), the module, the patch functions, and the fake-tensor paths.  The kernels themselves are
tests/test_mhstage_gpu.py."""
import ctypes
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

import mhstage_oracle
from conftest import ROOT, golden, golden_names

FIXTURES = golden_names("maskhead_")
# the reference's three ways to expand F images to N instances (devis_segmentation.py:35, deformable_segmentation.py:140-147)
EXPANDS = {
    "repeat": lambda t, n: t.repeat(n, 1, 1, 1),
    "interleaved": lambda t, n: t.unsqueeze(1).repeat(1, int(n), 1, 1, 1).flatten(0, 1),
    "ragged": lambda t, lengths: torch.cat([t[i].unsqueeze(0).repeat(1, int(k), 1, 1, 1).flatten(0, 1)
                                            for i, k in enumerate(lengths)], dim=0),
}


def load_fixture(name):
    """(arrays, state dict, features, bbox_mask), everything float64 (inputs and parameters are stored as float16, exact)."""
    d = {k: torch.from_numpy(v).double() for k, v in golden(name).items()}
    state = {k[len("state/"):]: v for k, v in d.items() if k.startswith("state/")}
    return d, state, [d["feature/%d" % i] for i in range(2)], [d["bbox_mask/%d" % i] for i in range(2)]


# ---- oracle ----------------------------------------------------------------------------------------------------------

def test_fixtures_cover_the_cases():
    assert FIXTURES == ["maskhead_interleaved", "maskhead_repeat"]
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 1 << 20
        d, state, features, bbox_mask = load_fixture(name)
        assert [tuple(f.shape) for f in features] == [(2, 64, 3, 5), (2, 24, 7, 9)]
        assert [tuple(b.shape) for b in bbox_mask] == [(6, 8, 3, 5), (6, 8, 7, 9)] and tuple(d["out"].shape) == (6, 1, 7, 9)
        assert [tuple(state["gn%d.weight" % i].shape) for i in (1, 2, 3)] == [(72,), (32,), (16,)]


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_equals_the_reference_outputs_and_gradients(name):
    d, state, features, bbox_mask = load_fixture(name)
    expand = EXPANDS[name.split("_")[1]]
    params = {n: p.clone().requires_grad_(True) for n, p in state.items()}
    features = [f.clone().requires_grad_(True) for f in features]
    bbox_mask = [b.clone().requires_grad_(True) for b in bbox_mask]

    # the reference's forward with every gn -> relu (-> interpolate -> add -> cat) written as one oracle stage
    def conv(nm, t, pad):
        return F.conv2d(t, params[nm + ".weight"], params[nm + ".bias"], padding=pad)

    def stage(nm, t, **kw):
        return mhstage_oracle.mask_head_stage(t, 8, params[nm + ".weight"], params[nm + ".bias"], **kw)

    x = torch.cat([expand(features[0], 3), bbox_mask[0]], 1)
    x = conv("lay2", stage("gn1", conv("lay1", x, 1)), 1)
    index = expand(torch.arange(2).view(2, 1, 1, 1), 3).flatten()
    x = stage("gn2", x, skip=conv("adapter1", features[1], 0), skip_index=index, extra=bbox_mask[1])
    out = conv("out_lay", stage("gn3", conv("lay3", x, 1)), 1)
    assert out.dtype == torch.float64 and float((out.detach() - d["out"]).abs().max()) <= 1e-12 * float(d["out"].abs().max())
    whole = mhstage_oracle.module_forward(state, features, bbox_mask, lambda t: expand(t, 3))
    assert float((whole.detach() - d["out"]).abs().max()) <= 1e-12 * float(d["out"].abs().max())
    grads = torch.autograd.grad(out, features + bbox_mask + list(params.values()), d["grad_out"])
    want = [d["grad/feature/%d" % i] for i in range(2)] + [d["grad/bbox_mask/%d" % i] for i in range(2)] + \
        [d["grad/state/" + n] for n in params]
    for g, w in zip(grads, want):
        assert float((g - w).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max()))


def test_oracle_gate_variant_equals_relu_for_its_own_gate():
    g = torch.Generator().manual_seed(4)
    x, w, b = torch.randn(2, 8, 3, 4, generator=g), torch.randn(8, generator=g), torch.randn(8, generator=g)
    z = mhstage_oracle.pre_activation(x, 2, w, b)
    a = mhstage_oracle.mask_head_stage(x, 2, w, b)
    assert torch.equal(a, mhstage_oracle.mask_head_stage(x, 2, w, b, gate=z > 0))
    gate, near = mhstage_oracle.device_gate(z, torch.zeros_like(z), 1e-5)
    assert near == 0 and torch.equal(gate, z > 0)
    gate, near = mhstage_oracle.device_gate(z, torch.ones_like(z), 10.0)
    assert near == z.numel() and bool(gate.all())


# ---- library ---------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_mhstage_h_declares_and_versions_agree():
    from devis_amd import _mhstage, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "mhstage.h")).read()
    declared = set(re.findall(r"\b(mhstage_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_mhstage.EXPORTED_SYMBOLS) and len(declared) == 6
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _mhstage.load()
    assert lib.mhstage_version() == _mhstage.MHSTAGE_ABI_VERSION == int(re.search(r"#define MHSTAGE_ABI_VERSION (\d+)", header).group(1))
    bits = tuple(int(re.search(r"#define MHSTAGE_GRAD_%s (\d+)" % n, header).group(1)) for n in ("X", "WEIGHT", "BIAS", "SKIP"))
    assert bits == (_mhstage.GRAD_X, _mhstage.GRAD_WEIGHT, _mhstage.GRAD_BIAS, _mhstage.GRAD_SKIP) == (1, 2, 4, 8)
    tiles = tuple(int(re.search(r"#define MHSTAGE_TILE_%s (\d+)" % n, header).group(1))
                  for n in ("STAT", "APPLY_PIXELS", "APPLY_CHANNELS", "BWD_PIXELS"))
    assert tiles == (_mhstage.TILE_STAT, _mhstage.TILE_APPLY_PIXELS, _mhstage.TILE_APPLY_CHANNELS, _mhstage.TILE_BWD_PIXELS)
    assert all(_mhstage.tile(t) > 0 and _mhstage.tile(t) % 32 == 0 for t in tiles) and lib.mhstage_tile(9) == -1
    codes = dict(re.findall(r"MHSTAGE_(F32|F64|BF16|F16) = (\d)", header))
    assert codes == {"F32": "0", "F64": "1", "BF16": "2", "F16": "3"}
    assert "floorf((float)d * ((float)h / (float)H))" in header         # the index rule is stated
    assert os.path.join(build.include_dir(), "mhstage.h") in build._headers()
    assert any(s.endswith("mhstage.hip") for s in build.sources())
    assert "mhstage.h" in open(os.path.join(ROOT, "setup.py")).read()


def _shape(**kw):
    from devis_amd import _mhstage
    d = dict(N=6, F=3, C=64, G=8, E=8, h=6, w=10, H=12, W=20)
    d.update(kw)
    return _mhstage.Shape(**d)


def test_mhstage_argument_errors_without_gpu():
    from devis_amd import _mhstage
    lib = _mhstage.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = ctypes.byref(_shape())
    err = lib.mhstage_last_error

    def fwd(dtype=0, wide=(0, 0, 0), x=p, weight=p, bias=p, skip=p, index=p, extra=p, shape=ok, ws=p, mean=p, rstd=p, out=p):
        return lib.mhstage_forward(dtype, wide[0], wide[1], wide[2], x, weight, bias, 1e-5, skip, index, 0, extra, shape, ws,
                                   mean, rstd, out, None)

    def bwd(grads=15, dtype=0, wide=(0, 0), x=p, go=p, layout=0, shape=ok, dy=p, gx=p, gw=p, gb=p, gs=p):
        return lib.mhstage_backward(grads, dtype, wide[0], wide[1], x, p, p, p, p, p, 0, go, layout, shape, p, dy, gx, gw, gb,
                                    gs, None)

    for name in ("x", "weight", "bias", "ws", "mean", "rstd", "out"):
        assert fwd(**{name: None}) == -1 and b"null pointer" in err(), name
    assert fwd(shape=None) == -1 and b"null pointer" in err()
    assert fwd(extra=None) == -1 and b"extra" in err()
    assert fwd(dtype=9) == -1 and b"dtype" in err()
    for dtype, wide in ((0, (1, 0, 0)), (1, (0, 0, 1)), (0, (0, 1, 0)), (2, (2, 0, 0))):
        assert fwd(dtype=dtype, wide=wide) == -1 and b"wide" in err(), (dtype, wide)
    for bad in (dict(C=0), dict(G=0), dict(h=0), dict(W=-1), dict(N=-1), dict(E=-1), dict(F=0)):
        assert fwd(shape=ctypes.byref(_shape(**bad))) == -1 and b"positive" in err(), bad
    assert fwd(shape=ctypes.byref(_shape(G=7))) == -1 and b"multiple" in err()
    assert fwd(shape=ctypes.byref(_shape(H=65536, W=65536))) == -1 and b"31 bits" in err()
    assert fwd(shape=ctypes.byref(_shape(h=65536, w=65536))) == -1 and b"31 bits" in err()
    assert fwd(shape=ctypes.byref(_shape(C=8, G=2, h=32768, w=32768))) == -1 and b"31 bits" in err()
    assert fwd(shape=ctypes.byref(_shape(C=2 ** 31 - 8, G=1, E=8))) == -1 and b"31 bits" in err()
    assert fwd(skip=None, extra=None, shape=ctypes.byref(_shape(E=0))) == -1 and b"H, W must be h, w" in err()
    assert fwd(skip=None, shape=ok) == -1 and b"skip_index without skip" in err()
    assert fwd(index=None, shape=ok) == -1 and b"must equal N" in err()
    assert fwd(x=None, weight=None, bias=None, skip=None, index=None, extra=None, ws=None, mean=None, rstd=None, out=None,
               shape=ctypes.byref(_shape(N=0, E=0, H=6, W=10))) == 0            # no image: nothing launched
    assert bwd(grads=16) == -1 and b"grads" in err()
    assert bwd(grads=0, x=None, go=None) == 0                                   # nothing asked for
    assert bwd(go=None) == -1 and b"null pointer" in err()
    assert bwd(x=None) == -1 and b"null pointer" in err()
    assert bwd(gx=None) == -1 and b"no buffer" in err()
    assert bwd(grads=8, gs=None) == -1 and b"no buffer" in err()
    assert bwd(grads=8, shape=ctypes.byref(_shape(F=0))) == -1 and b"positive" in err()
    assert bwd(layout=2) == -1 and b"layout" in err()
    assert bwd(dtype=2, wide=(0, 0), dy=p, gx=p) == -1 and b"alias" in err()
    assert bwd(dtype=0, wide=(1, 0)) == -1 and b"wide" in err()


def test_workspace_arithmetic():
    from devis_amd import _mhstage
    lib = _mhstage.load()
    stat, bp = _mhstage.tile(_mhstage.TILE_STAT), _mhstage.tile(_mhstage.TILE_BWD_PIXELS)
    up = lambda n: (n + 255) // 256 * 256      # noqa: E731

    def want(acc, N, C, G, h, w):
        fwd = N * G * -(-(C // G * h * w) // stat) * 2
        bwd = N * C * -(-(h * w) // bp) * 2 + N * C * 2 + N * G * 2
        return up(max(fwd, bwd) * acc)

    for dtype, acc in ((0, 4), (1, 8), (2, 4), (3, 4)):
        assert lib.mhstage_workspace_bytes(dtype, ctypes.byref(_shape())) == want(acc, 6, 64, 8, 6, 10)
        assert lib.mhstage_workspace_bytes(dtype, ctypes.byref(_shape(N=300, C=16, h=90, w=160))) == want(acc, 300, 16, 8, 90, 160)
    assert lib.mhstage_workspace_bytes(0, ctypes.byref(_shape(N=0))) == 0
    assert lib.mhstage_workspace_bytes(7, ctypes.byref(_shape())) == -1 and lib.mhstage_workspace_bytes(0, None) == -1
    with pytest.raises(RuntimeError, match="multiple"):
        _mhstage.workspace_bytes(0, _shape(G=5))


# ---- host ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", [(14, 46), (26, 22), (12, 23), (23, 45), (45, 90), (84, 167), (5, 5), (1, 7)])
def test_index_rule_restated_in_python_equals_f_interpolate(pair):
    from devis_amd import _mhstage
    a, A = pair
    want = F.interpolate(torch.arange(a, dtype=torch.float32).view(1, 1, a, 1), size=(A, 1), mode="nearest").flatten().long().tolist()
    got = [_mhstage.src_index(d, a, A) for d in range(A)]
    assert got == want
    if pair == (14, 46):
        assert got[23] != (23 * 14) // 46       # the integer rule is another rule


def test_operator_raises_on_cpu_tensors_and_on_bad_shapes_before_any_launch():
    import devis_amd
    from devis_amd.functions import mask_head_stage as S
    x, w, b = torch.zeros(6, 64, 6, 10), torch.ones(64), torch.zeros(64)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.mask_head_stage(x, 8, w, b)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        S._backward(torch.zeros(6, 64, 6, 10), x, w, b, torch.zeros(6, 8), torch.zeros(6, 8), None, 8, 0)
    assert devis_amd.mask_head_stage is devis_amd.ops.mask_head_stage
    for name in ("mask_head_stage", "MaskHeadConv", "patch_mask_head_stages", "unpatch_mask_head_stages"):
        assert name in devis_amd.__all__ and hasattr(devis_amd, name)

    meta = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="meta")      # noqa: E731
    x, w, b = meta(6, 64, 6, 10), meta(64), meta(64)
    f32, h = torch.float32, torch.bfloat16
    assert S.check_shapes(x, 8, w, b) == (6, 0, 64, 8, 0, 6, 10, 6, 10, f32)
    skip, idx, extra = meta(3, 64, 12, 20), meta(6, dtype=torch.int32), meta(6, 8, 12, 20)
    assert S.check_shapes(x, 8, w, b, skip, idx, extra) == (6, 3, 64, 8, 8, 6, 10, 12, 20, f32)
    assert S.check_shapes(x, 8, w, b, None, None, extra)[4:9] == (8, 6, 10, 12, 20)
    assert S.check_shapes(x, 8, w, b, meta(6, 64, 12, 20))[1] == 6
    xh = meta(6, 64, 6, 10, dtype=h)
    assert S.check_shapes(xh, 8, w, b, meta(3, 64, 12, 20, dtype=h), idx, extra, f32)[-1] == f32
    assert S.check_shapes(xh, 8, meta(64, dtype=h), meta(64, dtype=h))[-1] == h
    bad = [
        ("must be \\[N, C, h, w\\]", lambda: S.check_shapes(meta(64, 6, 10), 8, w, b)),
        ("multiple of the 7 groups", lambda: S.check_shapes(x, 7, w, b)),
        ("weight and bias must be", lambda: S.check_shapes(x, 8, meta(32), b)),
        ("weight must have x's dtype", lambda: S.check_shapes(x, 8, meta(64, dtype=h), meta(64, dtype=h))),
        ("bias must have weight's dtype", lambda: S.check_shapes(xh, 8, w, meta(64, dtype=h))),
        ("skip must be", lambda: S.check_shapes(x, 8, w, b, meta(3, 32, 12, 20), idx)),
        ("skip must have x's dtype", lambda: S.check_shapes(x, 8, w, b, meta(3, 64, 12, 20, dtype=h), idx)),
        ("without skip_index", lambda: S.check_shapes(x, 8, w, b, skip)),
        ("skip_index must be \\[N\\]", lambda: S.check_shapes(x, 8, w, b, skip, meta(5, dtype=torch.int64))),
        ("int32 or int64", lambda: S.check_shapes(x, 8, w, b, skip, meta(6))),
        ("skip_index without skip", lambda: S.check_shapes(x, 8, w, b, None, idx)),
        ("extra must be", lambda: S.check_shapes(x, 8, w, b, None, None, meta(5, 8, 12, 20))),
        ("extra must have x's dtype", lambda: S.check_shapes(x, 8, w, b, None, None, meta(6, 8, 12, 20, dtype=h))),
        ("disagree", lambda: S.check_shapes(x, 8, w, b, skip, idx, meta(6, 8, 12, 21))),
        ("out must have x's dtype", lambda: S.check_shapes(x, 8, w, b, out_dtype=h)),
        ("unsupported dtype", lambda: S.check_shapes(meta(6, 64, 6, 10, dtype=torch.int32), 8, w, b)),
    ]
    for match, call in bad:
        with pytest.raises(RuntimeError, match=match):
            call()


def test_needs_input_grad_maps_to_the_gradient_mask():
    from devis_amd import _mhstage, ops
    from devis_amd.functions import mask_head_stage as S
    from devis_amd.functions._common import op_runner
    assert S.grads_mask(True, False, False, False, False) == _mhstage.GRAD_X == S.NEED_X
    assert S.grads_mask(False, True, True, False, False) == _mhstage.GRAD_WEIGHT | _mhstage.GRAD_BIAS
    assert S.grads_mask(True, True, True, True, True) == S.NEED_ALL == 31 and _mhstage.GRAD_ALL == 15
    seen = []
    x, w, b = torch.zeros(6, 16, 3, 5), torch.zeros(16), torch.zeros(16)
    stats, go = torch.zeros(6, 8), torch.zeros(6, 20, 7, 9)

    def fake_op_backward(grad_out, x, weight, bias, mean, rstd, skip_index, num_groups, num_skip, grads):
        seen.append(("op", grads, num_groups, num_skip))
        return tuple(torch.zeros(1) if grads & bit else torch.zeros(0) for bit in (1, 2, 4, 8))

    def fake_host_backward(grad_out, x, weight, bias, mean, rstd, skip_index, num_groups, num_skip, grads):
        seen.append(("host", grads, num_groups, num_skip))
        return tuple(torch.zeros(1) if grads & bit else None for bit in (1, 2, 4, 8))

    # the one formula, run the way the op's register_autograd runs it and the way the eager Function does
    assert S.MaskHeadStageFunction.setup_context is S.setup_context is ops.mask_head_stage_op._setup_context_fn
    assert ops.mask_head_stage_op._backward_fn.func is S.backward
    T, N_ = True, False
    for needs, want in (((T, N_, T, T, N_, T, N_, T, N_), 31), ((T, N_, N_, N_, N_, N_, N_, N_, N_), 1),
                        ((N_, N_, T, T, N_, N_, N_, N_, N_), 6), ((N_, N_, N_, N_, N_, T, N_, T, N_), 24)):
        ctx = types.SimpleNamespace(saved_tensors=(x, w, b, stats, stats, None), needs_input_grad=needs, num_groups=8,
                                    num_skip=2, extra_dtype=torch.float32)
        for run, who in ((op_runner(fake_op_backward), "op"), (fake_host_backward, "host")):
            res = S.backward(run, ctx, go, None, None)
            assert seen[-1] == (who, want, 8, 2) and len(res) == 9
            assert tuple(r is not None for r in res) == needs
            if needs[7]:
                assert torch.equal(res[7], go[:, 16:])


# ---- module and patching ---------------------------------------------------------------------------------------------

def test_skip_index_from_the_reference_expand_functions():
    from devis_amd.modules import MaskHeadConv
    m = MaskHeadConv(64, [24], 8, False, [0, 1], 2)
    cpu = torch.device("cpu")
    assert m.skip_index(2, 3, EXPANDS["repeat"], cpu).tolist() == [0, 1, 0, 1, 0, 1]
    assert m.skip_index(2, 3, EXPANDS["interleaved"], cpu).tolist() == [0, 0, 0, 1, 1, 1]
    assert m.skip_index(3, [2, 0, 3], EXPANDS["ragged"], cpu).tolist() == [0, 0, 2, 2, 2]
    t = torch.randn(3, 4, 2, 2)
    for kind, n in (("repeat", 3), ("interleaved", 2), ("ragged", [1, 2, 3])):
        assert torch.equal(EXPANDS[kind](t, n), t[m.skip_index(3, n, EXPANDS[kind], cpu)])
    first = m.skip_index(2, 3, EXPANDS["repeat"], cpu)
    assert m.skip_index(2, 3, EXPANDS["repeat"], cpu) is first                  # cached per (F, instances, device)
    assert m.skip_index(2, 4, EXPANDS["repeat"], cpu).numel() == 8
    assert first.dtype == torch.int64 and "_index_cache" not in m.state_dict()


def _reference_shaped_head(dim, fpn_dims, nheads, maps, num_levels):
    """A module with the reference MaskHeadConv's parameter layout (plain convolutions), from its constructor's arithmetic."""
    out_dims = [dim // (2 ** e) for e in range(num_levels + 2)]
    in_dims = list(out_dims)
    for i in range(maps):
        in_dims[i] += nheads
    m = torch.nn.Module()
    m.lay1, m.gn1 = torch.nn.Conv2d(in_dims[0], in_dims[0], 3, padding=1), torch.nn.GroupNorm(8, in_dims[0])
    m.lay2, m.gn2 = torch.nn.Conv2d(in_dims[0], out_dims[1], 3, padding=1), torch.nn.GroupNorm(8, out_dims[1])
    for i in range(1, len(fpn_dims) + 1):
        setattr(m, "lay%d" % (i + 2), torch.nn.Conv2d(in_dims[i], out_dims[i + 1], 3, padding=1))
        setattr(m, "gn%d" % (i + 2), torch.nn.GroupNorm(8, out_dims[i + 1]))
        setattr(m, "adapter%d" % i, torch.nn.Conv2d(fpn_dims[i - 1], out_dims[i], 1))
    m.out_lay = torch.nn.Conv2d(out_dims[len(fpn_dims) + 1], 1, 3, padding=1)
    return m


def test_module_state_dict_initialisation_and_reference_checkpoint():
    from devis_amd.modules import MaskHeadConv, ModulatedDeformableConv2d
    m = MaskHeadConv(64, [24], 8, False, [0, 1], 2)
    theirs = _reference_shaped_head(64, [24], 8, 2, 2)
    assert list(m.state_dict()) == list(theirs.state_dict())
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in theirs.state_dict().items()}
    theirs.load_state_dict(m.state_dict(), strict=True)
    m.load_state_dict(theirs.state_dict(), strict=True)
    for name in FIXTURES:
        _, state, _, _ = load_fixture(name)
        md = MaskHeadConv(64, [24], 8, False, [0, 1], 2).double()
        md.load_state_dict(state, strict=True)
        assert torch.equal(md.lay3.weight, state["lay3.weight"])
    # the reference's plain convolution: kaiming-uniform with a = 1 (bound sqrt(3 / fan_in)), zero bias
    bound = (3.0 / (72 * 9)) ** 0.5
    assert 0.9 * bound < float(m.lay1.weight.detach().abs().max()) <= bound and float(m.lay1.bias.detach().abs().max()) == 0.0
    assert float(m.adapter1.bias.detach().abs().max()) == 0.0 and m.adapter1.kernel_size == (1, 1)
    assert m.multi_scale_att_maps and not MaskHeadConv(64, [24], 8, False, [0], 2).multi_scale_att_maps
    assert MaskHeadConv(64, [24], 8, False, [0, 1], 2, out_layer=False).out_lay is None
    big = MaskHeadConv(256, [256, 256, 256], 8, True, [0, 1, 2], 3)
    assert isinstance(big.lay1, ModulatedDeformableConv2d) and isinstance(big.out_lay, ModulatedDeformableConv2d)
    assert isinstance(big.adapter3, torch.nn.Conv2d) and [big.gn1.num_channels, big.gn2.num_channels, big.gn3.num_channels,
                                                          big.gn4.num_channels, big.gn5.num_channels] == [264, 128, 64, 32, 16]
    assert "lay1.regular_conv.weight" in big.state_dict() and "lay1.offset_conv.bias" in big.state_dict()


def test_patch_mask_head_stages_replaces_the_class_and_leaves_the_other_patches_alone():
    import devis_amd

    class Theirs(torch.nn.Module):
        pass

    class TheirConv(torch.nn.Module):
        pass

    class TheirMaps(torch.nn.Module):
        pass

    seg = types.SimpleNamespace(MaskHeadConv=Theirs, ModulatedDeformableConv2d=TheirConv, MultiScaleMHAttentionMap=TheirMaps)
    previous = devis_amd.patch_mask_head_stages(seg)
    assert previous is Theirs and seg.MaskHeadConv is devis_amd.modules.MaskHeadConv is devis_amd.MaskHeadConv
    assert seg.ModulatedDeformableConv2d is TheirConv and seg.MultiScaleMHAttentionMap is TheirMaps
    head = seg.MaskHeadConv(64, [24], 8, False, [0, 1], 2)
    assert isinstance(head, devis_amd.MaskHeadConv)
    devis_amd.unpatch_mask_head_stages(seg, previous)
    assert seg.MaskHeadConv is Theirs
    previous = devis_amd.patch_mask_head(seg)           # the convolution only, as before
    assert seg.MaskHeadConv is Theirs and seg.ModulatedDeformableConv2d is devis_amd.ModulatedDeformableConv2d
    devis_amd.argument_builders.unpatch_mask_head(seg, previous)
    previous = devis_amd.patch_attention_maps(seg)      # the maps only, as before
    assert seg.MaskHeadConv is Theirs and seg.ModulatedDeformableConv2d is TheirConv
    devis_amd.unpatch_attention_maps(seg, previous)
    with pytest.raises(AttributeError):
        devis_amd.patch_mask_head_stages(types.SimpleNamespace())


# ---- fake-tensor paths -----------------------------------------------------------------------------------------------

def _nodes(graph):
    return [n for n in graph.nodes if n.op == "call_function" and "mask_head_stage" in str(n.target)
            and "backward" not in str(n.target)]


def test_make_fx_with_fake_tensors_gives_one_op_node_with_channels_last_strides():
    from torch.fx.experimental.proxy_tensor import make_fx
    from devis_amd import ops
    meta = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")      # noqa: E731
    fn = lambda x, w, b, s, i, e: ops.mask_head_stage_op(x, 8, w, b, 1e-5, s, i, e)      # noqa: E731
    gm = make_fx(fn, tracing_mode="fake")(meta(6, 64, 6, 10), meta(64), meta(64), meta(3, 64, 12, 20),
                                          meta(6, dtype=torch.int64), meta(6, 8, 12, 20))
    nodes = _nodes(gm.graph)
    assert len(nodes) == 1
    out, mean, rstd = nodes[0].meta["val"]
    assert tuple(out.shape) == (6, 72, 12, 20) and out.stride() == (72 * 240, 1, 20 * 72, 72) and out.dtype == torch.float32
    assert tuple(mean.shape) == tuple(rstd.shape) == (6, 8) and mean.dtype == torch.float32
    h = torch.bfloat16
    fn = lambda x, w, b: ops.mask_head_stage_op(x, 8, w, b, 1e-5, None, None, None, torch.float32)      # noqa: E731
    out, mean, _ = _nodes(make_fx(fn, tracing_mode="fake")(meta(4, 16, 9, 11, dtype=h), meta(16), meta(16)).graph)[0].meta["val"]
    assert tuple(out.shape) == (4, 16, 9, 11) and out.stride() == (16 * 99, 1, 11 * 16, 16) and out.dtype == torch.float32
    fn = lambda x, w, b: ops.mask_head_stage_op(x, 8, w, b, 1e-5, None, None, None)      # noqa: E731
    out, mean, _ = _nodes(make_fx(fn, tracing_mode="fake")(meta(4, 16, 9, 11, dtype=torch.float64), meta(16, dtype=torch.float64),
                                                           meta(16, dtype=torch.float64)).graph)[0].meta["val"]
    assert out.dtype == mean.dtype == torch.float64
    gx, gw, gb, gs = ops._fake_mask_head_stage_backward(meta(6, 72, 12, 20), meta(6, 64, 6, 10), meta(64), meta(64), meta(6, 8),
                                                        meta(6, 8), None, 8, 3, 1 | 8)
    assert tuple(gx.shape) == (6, 64, 6, 10) and gw.numel() == 0 and gb.numel() == 0 and tuple(gs.shape) == (3, 64, 12, 20)


@pytest.mark.parametrize("dynamic", [False, True])
def test_export_gives_one_op_node_per_stage_for_static_and_dynamic_maps(dynamic):
    from devis_amd.modules import MaskHeadConv
    m = MaskHeadConv(64, [24], 8, False, [0, 1], 2).to("meta")

    class Wrap(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.m = m

        def forward(self, f0, f1, b0, b1):
            return self.m([f0, f1], [b0, b1], 3, EXPANDS["repeat"])

    meta = lambda *s: torch.empty(*s, device="meta")      # noqa: E731
    args = (meta(2, 64, 6, 10), meta(2, 24, 12, 20), meta(6, 8, 6, 10), meta(6, 8, 12, 20))
    shapes = None
    if dynamic:
        D = torch.export.Dim
        h, w, H, W = D("h", min=4, max=256), D("w", min=4, max=256), D("H", min=4, max=512), D("W", min=4, max=512)
        shapes = ({2: h, 3: w}, {2: H, 3: W}, {2: h, 3: w}, {2: H, 3: W})
    ep = torch.export.export(Wrap(), args, dynamic_shapes=shapes)
    nodes = _nodes(ep.graph)
    assert len(nodes) == 3          # gn1 plain, gn2 merged with the FPN level, gn3 plain
    val = nodes[1].meta["val"][0]
    assert val.shape[0] == 6 and val.shape[1] == 40 and len(val.shape) == 4
    if dynamic:
        assert not any(isinstance(val.shape[d], int) for d in (2, 3))
    else:
        assert tuple(val.shape) == (6, 40, 12, 20)
