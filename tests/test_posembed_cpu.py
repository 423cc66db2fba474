"""CPU tests of the encoder's positional input: the oracle against the reference fixtures, the C ABI of include/posembed.h
(exports, version, argument errors -- no compute calls), the host code (checks, errors), the modules' state dicts, the patch on
stand-in reference classes with the operators replaced by the oracle, and the fake-tensor paths.  The kernels themselves are
tests/test_posembed_gpu.py."""
import ctypes
import os
import re
import types

import pytest
import torch

import posembed_oracle
from conftest import ROOT, golden, golden_names

FIXTURES = golden_names("posembed_")
F32, F64 = torch.float32, torch.float64
SIZES = [(5, 7), (3, 4), (2, 2)]
RESULTS = ("src_flatten", "mask_flatten", "lvl_pos_embed_flatten", "spatial_shapes", "level_start_index", "valid_ratios")


def load_fixture(name):
    return {k: torch.from_numpy(v) for k, v in golden(name).items()}


def nested(mask, channels=1):
    """What the position encodings read of a NestedTensor."""
    return types.SimpleNamespace(tensors=torch.zeros(mask.shape[0], channels, *mask.shape[1:], device=mask.device), mask=mask)


# ---- stand-ins for the reference's classes: their text restated, the arithmetic through the oracle in float32 ---------------

class StockSine(torch.nn.Module):
    def __init__(self, num_pos_feats=64, temperature=10000, normalize=False, scale=None):
        super().__init__()
        self.num_pos_feats, self.temperature, self.normalize = num_pos_feats, temperature, normalize
        if scale is not None and normalize is False:
            raise ValueError("normalize should be True if scale is passed")
        self.scale = 2 * 3.141592653589793 if scale is None else scale

    def forward(self, tensor_list):
        return posembed_oracle.sine(tensor_list.mask, self.num_pos_feats, self.temperature, self.normalize, self.scale, F32)


class StockTransformer(torch.nn.Module):
    """level_embed, get_valid_ratio and a prepare_data that computes what deformable_transformer.py:60-94 computes."""

    def __init__(self, levels=3, channels=16):
        super().__init__()
        self.level_embed = torch.nn.Parameter(torch.randn(levels, channels))

    def get_valid_ratio(self, mask):
        return posembed_oracle.valid_ratio(mask)

    def prepare_data(self, srcs, masks, pos_embeds):
        tokens = lambda t: t.flatten(2).transpose(1, 2)      # noqa: E731
        src_flatten = torch.cat([tokens(s) for s in srcs], 1)
        mask_flatten = torch.cat([m.flatten(1) for m in masks], 1)
        lvl_pos_embed_flatten = torch.cat([tokens(p) + self.level_embed[lvl].view(1, 1, -1) for lvl, p in enumerate(pos_embeds)], 1)
        spatial_shapes = torch.as_tensor([tuple(s.shape[2:]) for s in srcs], dtype=torch.long, device=src_flatten.device)
        level_start_index = torch.cat((spatial_shapes.new_zeros((1,)), spatial_shapes.prod(1).cumsum(0)[:-1]))
        valid_ratios = torch.stack([self.get_valid_ratio(m) for m in masks], 1)
        return src_flatten, mask_flatten, lvl_pos_embed_flatten, spatial_shapes, level_start_index, valid_ratios


def reference_modules():
    """(position_encoding, deformable_transformer) namespaces with fresh stand-in classes, as the patches take them."""
    class PositionEmbeddingSine(StockSine):              # (inherits its forward: the patch has to cope with that)
        pass

    class PositionEmbeddingSineWithLearnableTemporal(PositionEmbeddingSine):
        def __init__(self, hidden_dim=256, num_frames=6, temperature=10000, normalize=False, scale=None):
            super().__init__(hidden_dim // 2, temperature, normalize, scale)
            self.num_frames = num_frames
            self.temporal_embed = torch.nn.Parameter(torch.randn(num_frames, hidden_dim))

        def forward(self, tensor_list):
            return super().forward(tensor_list) + self.temporal_embed[:, :, None, None]

    encoding = types.SimpleNamespace(PositionEmbeddingSine=PositionEmbeddingSine,
                                     PositionEmbeddingSineWithLearnableTemporal=PositionEmbeddingSineWithLearnableTemporal)
    encoder = type("DeformableTransformerEncoder", (), {"get_reference_points": staticmethod(lambda *a: "theirs")})
    transformer = types.SimpleNamespace(DeformableTransformer=type("DeformableTransformer", (StockTransformer,), {
        "prepare_data": StockTransformer.prepare_data}), DeformableTransformerEncoder=encoder)
    return encoding, transformer


def prepare_inputs(d, device="cpu"):
    """(srcs, masks, level_embed, temporal_embed) of the posembed_prepare fixture: srcs are recovered from src_flatten."""
    masks = [d["mask_%d" % l].to(device) for l in range(3)]
    srcs, at = [], 0
    for h, w in SIZES:
        srcs.append(d["src_flatten"][:, at:at + h * w].transpose(1, 2).reshape(3, 16, h, w).contiguous().to(device))
        at += h * w
    return srcs, masks, d["level_embed"].to(device), d["temporal_embed"].to(device)


def stand_in_model(encoding, transformer, d, device="cpu"):
    """(position encoding, transformer) instances holding the fixture's embeddings."""
    srcs, masks, level_embed, temporal_embed = prepare_inputs(d, device)
    pe = encoding.PositionEmbeddingSineWithLearnableTemporal(16, num_frames=3, normalize=True)
    top = transformer.DeformableTransformer()
    with torch.no_grad():
        pe.temporal_embed.copy_(temporal_embed)
        top.level_embed.copy_(level_embed)
    return pe.to(device), top.to(device), srcs, masks


# ---- oracle ------------------------------------------------------------------------------------------------------------------

def test_fixtures_cover_the_cases():
    assert FIXTURES == ["posembed_prepare", "posembed_sine", "posembed_temporal"]
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 32 << 10
    d = load_fixture("posembed_prepare")
    assert [tuple(d["mask_%d" % l].shape) for l in range(3)] == [(3,) + s for s in SIZES]
    assert tuple(d["lvl_pos_embed_flatten"].shape) == (3, 51, 16) and d["lvl_pos_embed_flatten"].dtype == F32
    assert d["spatial_shapes"].tolist() == [list(s) for s in SIZES] and d["level_start_index"].tolist() == [0, 35, 47]
    for l in range(3):
        m = d["mask_%d" % l]
        assert bool(m[2].all()) and not bool(m[0].all()) and not bool(m[1].all())         # one fully masked frame
    m = d["mask_0"]
    rect = lambda f: bool((f[:, f[0].logical_not()] == f[:, f[0].logical_not()][:, :1]).all())      # noqa: E731
    assert rect(m[0]) and not rect(m[1])                                                    # a rectangle; holes
    assert d["valid_ratios"][2].abs().max() == 0 and tuple(d["valid_ratios"].shape) == (3, 3, 2)


def test_oracle_equals_the_reference():
    d = load_fixture("posembed_sine")
    npf = int(d["num_pos_feats"])
    for key, kw in (("pos_plain", {}), ("pos_normalized", dict(normalize=True)),
                    ("pos_scaled", dict(temperature=20, normalize=True, scale=3.0))):
        assert torch.equal(posembed_oracle.sine(d["mask"], npf, dtype=F32, **kw), d[key]), key        # the same operations
        assert (posembed_oracle.sine(d["mask"], npf, dtype=F64, **kw) - d[key]).abs().max() < 5e-6, key
    t = load_fixture("posembed_temporal")
    pos = posembed_oracle.sine(t["mask"], 8, normalize=True, dtype=F32) + t["temporal_embed"][:, :, None, None]
    assert torch.equal(pos, t["pos"])
    p = load_fixture("posembed_prepare")
    _, masks, level_embed, temporal_embed = prepare_inputs(p)
    got = posembed_oracle.encoder(masks, level_embed, temporal_embed, dtype=F32)
    for g, key in zip(got, ("lvl_pos_embed_flatten", "mask_flatten", "valid_ratios")):
        assert g.dtype == p[key].dtype and torch.equal(g, p[key]), key
    wide = posembed_oracle.encoder(masks, level_embed.double(), temporal_embed.double())[0]
    assert wide.dtype == F64 and (wide - p["lvl_pos_embed_flatten"]).abs().max() < 5e-6
    # the kernels' arithmetic after the sine values is the reference's: the two-rounding form with no rounding is the tail
    flat = posembed_oracle.flat_sine(masks, 8, dtype=F32)
    assert torch.equal(posembed_oracle.embed_rounded(flat, SIZES, level_embed, temporal_embed, None, F32), p["lvl_pos_embed_flatten"])
    for lvl in range(3):
        assert torch.equal(posembed_oracle.sine(masks[lvl], 8, normalize=True, dtype=F32) + temporal_embed[:, :, None, None],
                           p["pos_%d" % lvl])
    g = torch.randn(3, 51, 16, dtype=F64)
    lv, tp = level_embed.double().requires_grad_(True), temporal_embed.double().requires_grad_(True)
    (posembed_oracle.encoder(masks, lv, tp)[0] * g).sum().backward()
    want = posembed_oracle.embedding_gradients(g, SIZES)
    assert torch.allclose(lv.grad, want[0], atol=1e-12) and torch.allclose(tp.grad, want[1], atol=1e-12)
    cy, cx, ty, tx = posembed_oracle.counts(masks[0])
    assert torch.equal(cy[:, -1], ty) and torch.equal(cx[:, :, -1], tx) and int(cy[2].max()) == 0


# ---- library -----------------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_posembed_h_declares_and_versions_agree():
    from devis_amd import _posembed, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "posembed.h")).read()
    declared = set(re.findall(r"\b(posembed_[a-z_0-9]+)\s*\(", header.split("#ifndef POSEMBED_H")[1]))
    assert declared == set(_posembed.EXPORTED_SYMBOLS) and len(declared) == 8
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _posembed.load()
    assert lib.posembed_version() == _posembed.POSEMBED_ABI_VERSION == 1 == int(re.search(r"#define POSEMBED_ABI_VERSION (\d+)", header).group(1))
    assert dict(re.findall(r"POSEMBED_(F32|F64|BF16|F16) = (\d)", header)) == {"F32": "0", "F64": "1", "BF16": "2", "F16": "3"}
    for name, value in (("TILE_TOKENS", _posembed.TILE_TOKENS), ("TILE_CHANNELS", _posembed.TILE_CHANNELS),
                        ("TILE_PIXELS", _posembed.TILE_PIXELS), ("WS_COUNTS", _posembed.WS_COUNTS),
                        ("WS_BACKWARD", _posembed.WS_BACKWARD), ("MAX_LEVELS", _posembed.MAX_LEVELS)):
        assert int(re.search(r"#define POSEMBED_%s (\d+)" % name, header).group(1)) == value, name
    assert _posembed.tile(_posembed.TILE_TOKENS) > 0 and _posembed.tile(_posembed.TILE_PIXELS) == 64
    assert lib.posembed_tile(7) == -1 and lib.posembed_tile(-1) == -1
    assert ctypes.sizeof(_posembed.Shape) == 4 * (3 + 2 * 8) and ctypes.sizeof(_posembed.Masks) == 8 * 4 * 8
    from devis_amd import _native
    assert _native.load().msda_build_info().decode() == "abi=14 arch=gfx950"              # no other ABI moved
    assert os.path.join(build.include_dir(), "posembed.h") in build._headers()
    assert any(s.endswith("posembed.hip") for s in build.sources())
    assert "posembed.h" in open(os.path.join(ROOT, "setup.py")).read() and "posembed.h" in build.include_dir.__doc__


def test_posembed_argument_errors_without_gpu():
    from devis_amd import _posembed
    lib = _posembed.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.posembed_last_error

    def shape(N=3, sizes=SIZES, C=16):
        s = _posembed.Shape(N=N, L=len(sizes), C=C)
        for l, (h, w) in enumerate(sizes[:_posembed.MAX_LEVELS]):
            s.H[l], s.W[l] = h, w
        return ctypes.byref(s)

    masks = _posembed.Masks()
    for l in range(3):
        masks.ptr[l] = p.value
    flat = lambda dtype=0, ws=p, shape=shape(), dim_t=p, lv=p, tp=p, norm=1, scale=6.28, rd=-1, pos=p: lib.posembed_write_flat(      # noqa: E731
        dtype, ws, shape, dim_t, lv, tp, norm, scale, rd, pos, None)
    nchw = lambda dtype=0, ws=p, shape=shape(sizes=SIZES[:1]), dim_t=p, norm=1, scale=6.28, pos=p: lib.posembed_write_nchw(       # noqa: E731
        dtype, ws, shape, dim_t, norm, scale, pos, None)
    bwd = lambda dtype=0, grad=p, shape=shape(), ws=p, gl=p, gt=p: lib.posembed_backward(dtype, grad, shape, ws, gl, gt, None)   # noqa: E731
    cnt = lambda m=ctypes.byref(masks), shape=shape(), ws=p, mf=p, vr=p: lib.posembed_counts(m, shape, ws, mf, vr, None)          # noqa: E731
    for call in (flat, nchw, bwd):
        assert call(dtype=9) == -1 and b"dtype" in err()
        assert call(dtype=1) == -1 and b"dtype" in err()                    # float64 is refused
        assert call(shape=None) == -1 and b"null pointer" in err()
        assert call(shape=shape(C=14)) == -1 and b"num_pos_feats" in err()  # an odd num_pos_feats
        assert call(shape=shape(C=0)) == -1 and b"num_pos_feats" in err()
    for call in (flat, nchw, bwd, cnt):
        assert call(shape=shape(N=-1)) == -1 and b"negative" in err()
        assert call(shape=shape(sizes=[])) == -1 and b"outside" in err()
        assert call(shape=shape(sizes=[(1, 1)] * 9)) == -1 and b"outside" in err()
        assert call(shape=shape(sizes=[(5, 0)])) == -1 and b"positive" in err()
        assert call(shape=shape(sizes=[(1 << 16, 1 << 16)])) == -1 and b"31 bits" in err()
        assert call(shape=shape(N=1 << 20, sizes=[(1 << 10, 1 << 10)])) == -1 and b"31 bits" in err()
    assert flat(rd=0) == -1 and b"round_dtype" in err() and flat(rd=1) == -1 and flat(scale=float("nan")) == -1 and b"scale" in err()
    assert nchw(shape=shape()) == -1 and b"one level" in err()
    for name in ("ws", "dim_t", "lv", "pos"):
        assert flat(**{name: None}) == -1 and b"null pointer" in err(), name
    assert flat(pos=ctypes.c_void_p(p.value + 4)) == -1 and b"16-byte" in err()
    for name in ("ws", "dim_t", "pos"):
        assert nchw(**{name: None}) == -1 and b"null pointer" in err(), name
    assert bwd(gl=None, gt=None) == -1 and b"one of the two" in err()
    assert bwd(grad=None) == -1 and b"null pointer" in err() and bwd(ws=None) == -1
    assert cnt(m=None) == -1 and cnt(ws=None) == -1 and b"workspace" in err()
    assert cnt(m=ctypes.byref(_posembed.Masks())) == -1 and b"level 0" in err()
    # nothing to compute: nothing is launched, nothing is dereferenced
    assert flat(ws=None, dim_t=None, lv=None, tp=None, pos=None, shape=shape(N=0)) == 0
    assert nchw(ws=None, dim_t=None, pos=None, shape=shape(N=0, sizes=SIZES[:1])) == 0
    assert cnt(m=ctypes.byref(_posembed.Masks()), ws=None, mf=None, vr=None, shape=shape(N=0)) == 0
    # the workspaces: host arithmetic
    ws = lambda which, **kw: lib.posembed_workspace_bytes(which, shape(**kw))      # noqa: E731
    tokens = _posembed.tile(_posembed.TILE_TOKENS)
    assert ws(0) % 256 == 0 and ws(0) >= 4 * 3 * (2 * 51 + 13 + 10) and ws(0, N=0) == 0
    assert ws(1) == 3 * 3 * 16 * 4 + (256 - 3 * 3 * 16 * 4 % 256) % 256                                 # one chunk per level
    assert ws(1, N=1, sizes=[(1, tokens + 1)], C=4) == 256 and ws(1, N=1, sizes=[(1, tokens + 1)], C=64) == 512
    assert ws(2) == -1 and b"workspace code" in err() and ws(1, C=14) == -1 and lib.posembed_workspace_bytes(0, None) == -1


def test_operators_raise_on_cpu_tensors_and_on_bad_arguments_before_any_launch(monkeypatch):
    import devis_amd
    from devis_amd import _posembed
    from devis_amd.functions import position_embedding as P

    def no_launch(*a, **k):
        raise AssertionError("a kernel call was made")

    for name in ("counts", "write_flat", "write_nchw", "backward"):
        monkeypatch.setattr(_posembed, name, no_launch)
    masks = [torch.zeros(3, h, w, dtype=torch.bool) for h, w in SIZES]
    level, temporal = torch.zeros(3, 16), torch.zeros(3, 16)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.sine_position_embedding(masks[0], num_pos_feats=8)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.encoder_position_embedding(masks, level, temporal)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        P._encoder_backward(torch.zeros(3, 51, 16), [5, 3, 2], [7, 4, 2], True, True)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        P.counts(masks)
    names = ("sine_position_embedding", "encoder_position_embedding", "DeferredPositionEmbedding", "patch_position_encoding",
             "unpatch_position_encoding")
    for name in names:
        assert name in devis_amd.__all__ and hasattr(devis_amd, name)
    assert devis_amd.sine_position_embedding is devis_amd.ops.sine_position_embedding
    assert devis_amd.patch_position_encoding is devis_amd.argument_builders.patch_position_encoding
    assert "no CPU path" in P.__doc__

    meta = lambda *s, dtype=F32: torch.zeros(*s, dtype=dtype, device="meta")      # noqa: E731
    mm = [meta(3, h, w, dtype=torch.bool) for h, w in SIZES]
    ok = P.check_encoder(mm, meta(3, 16), meta(3, 16), None, True, None, None, None)
    assert ok[:4] == (3, SIZES, 16, 8) and abs(ok[4] - 6.283185307179586) < 1e-15 and ok[5] == F32
    assert P.check_encoder(mm, meta(3, 16), None, 8, True, 3.0, torch.bfloat16, None)[4:] == (3.0, F32)           # torch's promotion
    assert P.check_encoder(mm, meta(3, 16, dtype=torch.float16), None, 8, False, None, None, None)[5] == F32
    assert P.check_encoder(mm, meta(3, 16, dtype=torch.float16), None, 8, False, None, torch.float16, None)[5] == torch.float16
    assert P.check_encoder(mm, meta(3, 16), None, 8, True, None, torch.float16, torch.float16)[5] == torch.float16
    assert P.check_sine(mm[0], 8, False, None, None) == (3, (5, 7), 6.283185307179586, F32)
    strided = torch.zeros(3, 7, 5, dtype=torch.bool, device="meta").transpose(1, 2)
    assert P.check_masks("x", [strided]) == (3, [(5, 7)])                                                  # any strides
    bad = [
        (RuntimeError, "must be bool", lambda: P.check_sine(meta(3, 5, 7, dtype=torch.uint8), 8, False, None, None)),
        (RuntimeError, "must be bool", lambda: P.check_encoder([meta(3, 5, 7)] + mm[1:], meta(3, 16), None, None, True, None, None, None)),
        (RuntimeError, r"must be \[N, H, W\]", lambda: P.check_sine(meta(5, 7, dtype=torch.bool), 8, False, None, None)),
        (RuntimeError, "num_pos_feats must be even", lambda: P.check_sine(mm[0], 7, False, None, None)),
        (RuntimeError, "num_pos_feats must be even", lambda: P.check_encoder(mm, meta(3, 14), None, None, True, None, None, None)),
        (ValueError, "normalize should be True if scale is passed", lambda: P.check_sine(mm[0], 8, False, 2.0, None)),
        (ValueError, "normalize should be True if scale is passed", lambda: P.check_encoder(mm, meta(3, 16), None, None, False, 2.0, None, None)),
        (RuntimeError, "level_embed has 16 channels, 2 \\* num_pos_feats is 12", lambda: P.check_encoder(mm, meta(3, 16), None, 6, True, None, None, None)),
        (RuntimeError, "temporal_embed has 2 frames, the masks 3", lambda: P.check_encoder(mm, meta(3, 16), meta(2, 16), None, True, None, None, None)),
        (RuntimeError, "temporal_embed has 12 channels", lambda: P.check_encoder(mm, meta(3, 16), meta(3, 12), None, True, None, None, None)),
        (RuntimeError, "3 masks, but level_embed has 4 levels", lambda: P.check_encoder(mm, meta(4, 16), None, None, True, None, None, None)),
        (RuntimeError, "level 1 has 2 frames, level 0 3", lambda: P.check_encoder([mm[0], meta(2, 3, 4, dtype=torch.bool)], meta(2, 16), None, None, True, None, None, None)),
        (RuntimeError, "1 to 8 levels", lambda: P.check_encoder([], meta(0, 16), None, None, True, None, None, None)),
        (RuntimeError, "round_dtype must be", lambda: P.check_encoder(mm, meta(3, 16), None, None, True, None, F32, None)),
        (RuntimeError, "out_dtype must be", lambda: P.check_encoder(mm, meta(3, 16), None, None, True, None, None, F64)),
        (RuntimeError, "out_dtype must be", lambda: P.check_encoder(mm, meta(3, 16, dtype=F64), None, None, True, None, None, None)),
        (RuntimeError, "out_dtype must be", lambda: P.check_sine(mm[0], 8, False, None, torch.int32)),
    ]
    for kind, match, call in bad:
        with pytest.raises(kind, match=match):
            call()
    with pytest.raises(ValueError, match="normalize should be True"):            # the public functions run the same checks
        devis_amd.sine_position_embedding(masks[0], num_pos_feats=8, scale=2.0)
    with pytest.raises(RuntimeError, match="temporal_embed has 2 frames"):
        devis_amd.encoder_position_embedding(masks, level, torch.zeros(2, 16))


def test_only_the_requested_gradient_is_computed():
    from devis_amd import ops
    from devis_amd.functions import position_embedding as P
    seen = []

    def fake(grad, heights, widths, want_level, want_temporal):
        seen.append((list(heights), list(widths), want_level, want_temporal))
        return torch.zeros(3, 16) if want_level else torch.zeros(0), torch.zeros(3, 16) if want_temporal else torch.zeros(0)

    # the one formula, for the eager Function's argument order (the embeddings first, the masks last and one by one) and for
    # the op's (the masks first, as a list)
    assert ops.encoder_position_embedding_op._setup_context_fn is P.setup_context
    assert ops.encoder_position_embedding_op._backward_fn.func is P.backward
    g = torch.ones(3, 51, 16)
    for level, temporal, has_temporal in ((True, True, True), (True, False, True), (False, True, True), (False, False, True), (True, True, False)):
        dtypes = (F32, torch.float16 if has_temporal else None)
        eager = types.SimpleNamespace(mark_non_differentiable=lambda *t: None)
        P.EncoderPositionEmbeddingFunction.setup_context(
            eager, (torch.zeros(3, 16), torch.zeros(3, 16, dtype=torch.float16) if has_temporal else None) + (None,) * 6 +
            tuple(torch.zeros((3,) + s, dtype=torch.bool) for s in SIZES), (None, None, None))
        assert (eager.heights, eager.widths, eager.dtypes) == ([5, 3, 2], [7, 4, 2], dtypes)
        eager.needs_input_grad = (level, temporal) + (False,) * 9
        op = types.SimpleNamespace(heights=[5, 3, 2], widths=[7, 4, 2], dtypes=dtypes, needs_input_grad=(False, level, temporal) + (False,) * 6)
        before = len(seen)
        a = P.backward(fake, eager, g, None, None, embeds_at=0)
        b = P.backward(fake, op, g, None, None)
        assert len(a) == 11 and len(b) == 9 and b[0] is None
        want_t = temporal and has_temporal
        for gl, gt in ((a[0], a[1]), (b[1], b[2])):
            assert (gl is not None) == level and (gt is not None) == want_t
            assert gt is None or gt.dtype == torch.float16                       # in the embedding's dtype
        assert all(r is None for r in a[2:] + b[3:])
        assert seen[before:] == ([([5, 3, 2], [7, 4, 2], level, want_t)] * 2 if level or want_t else [])


def test_the_formula_runs_under_torchs_autograd_for_the_function_and_for_the_op(monkeypatch):
    """Both registrations of the one formula through torch's own machinery, with the kernel launches stubbed out: the
    Function's masks are separate arguments, the op's are a list, whose gradient slot has to be a list of None."""
    from devis_amd import _posembed, ops
    from devis_amd.functions import position_embedding as P
    monkeypatch.setattr(P, "_check_device", lambda *a: None)
    monkeypatch.setattr(_posembed, "workspace_bytes", lambda *a: 16)
    for name in ("counts", "write_flat", "backward"):
        monkeypatch.setattr(_posembed, name, lambda *a, **k: None)
    masks = [torch.zeros((3,) + s, dtype=torch.bool) for s in SIZES]
    rest = (None, 10000.0, True, None, None, None)
    for call in (lambda lv, tp: P.EncoderPositionEmbeddingFunction.apply(lv, tp, *rest, *masks),
                 lambda lv, tp: ops.encoder_position_embedding_op(masks, lv, tp, *rest)):
        level = torch.zeros(3, 16, requires_grad=True)
        temporal = torch.zeros(3, 16, dtype=torch.float64, requires_grad=True)
        pos, mask_flatten, valid_ratios = call(level, temporal)
        assert pos.requires_grad and not mask_flatten.requires_grad and not valid_ratios.requires_grad
        grad_level, grad_temporal = torch.autograd.grad(pos.sum(), [level, temporal])
        assert (grad_level.dtype, grad_temporal.dtype) == (F32, torch.float64)


# ---- modules and patches -----------------------------------------------------------------------------------------------------

def test_modules_take_the_references_arguments_and_state_dicts():
    from devis_amd import modules
    sine = modules.PositionEmbeddingSine(8, 20, True, 3.0)
    assert (sine.num_pos_feats, sine.temperature, sine.normalize, sine.scale) == (8, 20, True, 3.0) and not sine.state_dict()
    assert modules.PositionEmbeddingSine().scale == 2 * 3.141592653589793 and modules.PositionEmbeddingSine().num_pos_feats == 64
    with pytest.raises(ValueError, match="normalize should be True"):
        modules.PositionEmbeddingSine(8, scale=2.0)
    t = load_fixture("posembed_temporal")
    temporal = modules.PositionEmbeddingSineWithLearnableTemporal(16, num_frames=3, normalize=True)
    assert isinstance(temporal, modules.PositionEmbeddingSine) and temporal.num_pos_feats == 8 and temporal.num_frames == 3
    assert list(temporal.state_dict()) == ["temporal_embed"] and tuple(temporal.temporal_embed.shape) == (3, 16)
    temporal.load_state_dict({"temporal_embed": t["temporal_embed"]})                       # the reference's key
    assert torch.equal(temporal.temporal_embed, t["temporal_embed"]) and temporal.temporal_embed.requires_grad
    assert modules.PositionEmbeddingSineWithLearnableTemporal().temporal_embed.shape == (6, 256)


def test_module_forward_is_the_nchw_operator_plus_the_temporal_embedding(monkeypatch):
    import devis_amd
    from devis_amd import modules, ops
    t = load_fixture("posembed_temporal")
    calls = []

    def oracle(mask, **kw):
        calls.append(kw)
        return posembed_oracle.sine(mask, kw["num_pos_feats"], kw["temperature"], kw["normalize"], kw["scale"], F32)

    monkeypatch.setattr(ops, "sine_position_embedding", oracle)
    temporal = modules.PositionEmbeddingSineWithLearnableTemporal(16, num_frames=3, normalize=True)
    temporal.load_state_dict({"temporal_embed": t["temporal_embed"]})
    pos = temporal(nested(t["mask"]))
    assert torch.equal(pos, t["pos"]) and pos.requires_grad and calls == [dict(num_pos_feats=8, temperature=10000, normalize=True, scale=2 * 3.141592653589793)]
    pos.sum().backward()
    assert torch.equal(temporal.temporal_embed.grad, torch.full((3, 16), 35.0))
    s = load_fixture("posembed_sine")
    assert torch.equal(modules.PositionEmbeddingSine(8)(nested(s["mask"])), s["pos_plain"]) and calls[-1]["scale"] is None
    # deferred: nothing runs until it is needed
    temporal.deferred = True
    before = len(calls)
    deferred = temporal(nested(t["mask"]))
    assert isinstance(deferred, devis_amd.DeferredPositionEmbedding) and len(calls) == before
    assert deferred.shape == torch.Size((3, 16, 5, 7)) and deferred.module is temporal and deferred.mask is t["mask"] and deferred.dtype is None
    half = deferred.to(torch.float16)
    assert isinstance(half, devis_amd.DeferredPositionEmbedding) and half.dtype == torch.float16 and len(calls) == before
    assert torch.equal(half.materialize(), t["pos"].to(torch.float16)) and half.materialize() is half.materialize()
    assert torch.equal(deferred.flatten(2), t["pos"].flatten(2)) and deferred.dim() == 4 and len(calls) == before + 2
    assert torch.equal(deferred.to("cpu", torch.float64), t["pos"].double())


def test_patch_sets_and_restores_and_leaves_the_other_patches_alone_in_both_orders():
    import devis_amd
    from devis_amd import argument_builders as AB
    from devis_amd.modules import position_encoding as PE
    for transformer_first in (True, False):
        encoding, transformer = reference_modules()
        top, sine, temporal = transformer.DeformableTransformer, encoding.PositionEmbeddingSine, encoding.PositionEmbeddingSineWithLearnableTemporal
        theirs = (top.__dict__["prepare_data"], sine.forward, temporal.forward, transformer.DeformableTransformerEncoder.__dict__["get_reference_points"])
        existing = temporal(16, 3)
        if transformer_first:
            undo_t = devis_amd.patch_transformer(transformer)
            assert top.prepare_data is AB.prepare_data
        undo_p = devis_amd.patch_position_encoding(encoding, transformer)
        assert sine.forward is PE.deferred_forward and temporal.forward is PE.deferred_forward
        assert top.prepare_data is AB.prepare_data_deferred
        assert isinstance(existing(nested(torch.zeros(3, 2, 2, dtype=torch.bool))), devis_amd.DeferredPositionEmbedding)       # modules that exist follow
        assert undo_p["prepare_data"] is (AB.prepare_data if transformer_first else theirs[0])
        if not transformer_first:
            assert transformer.DeformableTransformerEncoder.get_reference_points("a", "b", "c") == "theirs"
            undo_t = devis_amd.patch_transformer(transformer)
            assert top.prepare_data is AB.prepare_data                              # the documented order: nothing is fused now
            assert sine.forward is PE.deferred_forward
            AB.unpatch_transformer(transformer, undo_t)
            assert top.prepare_data is AB.prepare_data_deferred
        assert transformer.DeformableTransformerEncoder.get_reference_points is (AB.get_reference_points if transformer_first else theirs[3].__func__)
        devis_amd.unpatch_position_encoding(encoding, transformer, undo_p)
        assert (sine.forward, temporal.forward) == theirs[1:3]
        if transformer_first:
            assert top.prepare_data is AB.prepare_data
            AB.unpatch_transformer(transformer, undo_t)
        assert top.__dict__["prepare_data"] is theirs[0] and "_devis_amd_prepare_data" not in top.__dict__
        assert transformer.DeformableTransformerEncoder.__dict__["get_reference_points"] is theirs[3]
    with pytest.raises(AttributeError):
        devis_amd.patch_position_encoding(types.SimpleNamespace(), types.SimpleNamespace())
    assert "EAGER ONLY" in devis_amd.patch_position_encoding.__doc__ and "FIRST" in devis_amd.patch_position_encoding.__doc__


def oracle_operators(monkeypatch, calls):
    """The two public operators replaced by the float32 oracle on the tensors' own device; ``calls`` counts them."""
    from devis_amd import ops

    def sine(mask, *, num_pos_feats, temperature=10000, normalize=False, scale=None, out_dtype=None):
        calls.append("sine")
        return posembed_oracle.sine(mask, num_pos_feats, temperature, normalize, scale, F32)

    def encoder(masks, level_embed, temporal_embed=None, *, num_pos_feats=None, temperature=10000, normalize=True, scale=None,
                round_dtype=None, out_dtype=None):
        calls.append("encoder")
        return posembed_oracle.encoder(masks, level_embed, temporal_embed, num_pos_feats, temperature, normalize, scale, round_dtype, F32)

    monkeypatch.setattr(ops, "sine_position_embedding", sine)
    monkeypatch.setattr(ops, "encoder_position_embedding", encoder)


def check_six(got, d, exact=True, tol=0.0):
    assert len(got) == 6
    for g, key in zip(got, RESULTS):
        want = d[key].to(g.device)
        assert g.dtype == want.dtype and g.shape == want.shape, key
        if key == "lvl_pos_embed_flatten" and not exact:
            assert float((g.detach() - want).abs().max()) <= tol, (key, float((g.detach() - want).abs().max()))
        elif key == "valid_ratios" and not exact:       # (the device multiplies by the reciprocal: tests/test_posembed_gpu.py)
            assert float((g - want).abs().max()) <= 2.0 ** -23, key
        else:
            assert torch.equal(g.detach(), want), key


def test_a_deferred_embedding_handed_to_the_stock_prepare_data_gives_the_stock_result(monkeypatch):
    import devis_amd
    d = load_fixture("posembed_prepare")
    calls = []
    oracle_operators(monkeypatch, calls)
    encoding, transformer = reference_modules()
    pe, top, srcs, masks = stand_in_model(encoding, transformer, d)
    check_six(top.prepare_data(srcs, masks, [pe(nested(m)).to(F32) for m in masks]), d)                # the stand-ins are the reference
    undo = devis_amd.patch_position_encoding(encoding, transformer)
    try:
        pos = [pe(nested(m)).to(F32) for m in masks]
        assert all(isinstance(p, devis_amd.DeferredPositionEmbedding) for p in pos) and calls == []
        check_six(StockTransformer.prepare_data(top, srcs, masks, pos), d)                             # a consumer that knows nothing
        assert calls == ["sine"] * 3
        # the fused route: one call
        del calls[:]
        got = top.prepare_data(srcs, masks, [pe(nested(m)).to(F32) for m in masks])
        check_six(got, d)
        assert calls == ["encoder"] and got[3] is devis_amd.argument_builders.interned_pyramid(SIZES, "cpu")[0]
        got[2].sum().backward()
        assert top.level_embed.grad is not None and pe.temporal_embed.grad is not None
        # not fusable: a plain tensor among them, or another module's embedding -- materialised, the existing route
        del calls[:]
        mixed = [pe(nested(m)).to(F32) for m in masks]
        mixed[1] = mixed[1].materialize()
        check_six(top.prepare_data(srcs, masks, mixed), d)
        assert calls == ["sine"] * 3
        other = encoding.PositionEmbeddingSineWithLearnableTemporal(16, num_frames=3, normalize=True)
        other.load_state_dict(pe.state_dict())
        del calls[:]
        check_six(top.prepare_data(srcs, masks, [pe(nested(masks[0])), other(nested(masks[1])), pe(nested(masks[2]))]), d)
        assert calls == ["sine"] * 3
        # both orders with patch_transformer give the right results; this one is not fused
        undo_t = devis_amd.patch_transformer(transformer)
        del calls[:]
        check_six(top.prepare_data(srcs, masks, [pe(nested(m)).to(F32) for m in masks]), d)
        assert calls == ["sine"] * 3
        devis_amd.argument_builders.unpatch_transformer(transformer, undo_t)
    finally:
        devis_amd.unpatch_position_encoding(encoding, transformer, undo)
    # ... and patch_transformer first, then this patch: fused
    undo_t = devis_amd.patch_transformer(transformer)
    undo = devis_amd.patch_position_encoding(encoding, transformer)
    try:
        del calls[:]
        check_six(top.prepare_data(srcs, masks, [pe(nested(m)).to(F32) for m in masks]), d)
        assert calls == ["encoder"]
    finally:
        devis_amd.unpatch_position_encoding(encoding, transformer, undo)
        devis_amd.argument_builders.unpatch_transformer(transformer, undo_t)


# ---- fake-tensor paths -------------------------------------------------------------------------------------------------------

def _nodes(graph, name):
    return [n for n in graph.nodes if n.op == "call_function" and name in str(n.target) and "backward" not in str(n.target)]


def test_make_fx_with_fake_tensors_gives_one_op_node():
    from torch.fx.experimental.proxy_tensor import make_fx
    from devis_amd import ops
    meta = lambda *s, dtype=F32: torch.empty(*s, dtype=dtype, device="meta")      # noqa: E731
    for out in (None, torch.bfloat16, torch.float16):
        gm = make_fx(lambda m: ops.sine_position_embedding_op(m, 8, 10000.0, True, None, out), tracing_mode="fake")(
            meta(3, 5, 7, dtype=torch.bool))
        node, = _nodes(gm.graph, "sine_position_embedding")
        assert tuple(node.meta["val"].shape) == (3, 16, 5, 7) and node.meta["val"].dtype == (out or F32)
    for rd, temporal in ((None, True), (torch.bfloat16, True), (None, False)):
        fn = ((lambda a, b, c, lv, tp: ops.encoder_position_embedding_op([a, b, c], lv, tp, None, 10000.0, True, None, rd, None)) if temporal
              else (lambda a, b, c, lv: ops.encoder_position_embedding_op([a, b, c], lv, None, None, 10000.0, True, None, rd, None)))
        args = [meta(3, h, w, dtype=torch.bool) for h, w in SIZES] + [meta(3, 16)] + ([meta(3, 16)] if temporal else [])
        gm = make_fx(fn, tracing_mode="fake")(*args)
        node, = _nodes(gm.graph, "encoder_position_embedding")
        pos, flat, ratios = node.meta["val"]
        assert tuple(pos.shape) == (3, 51, 16) and pos.dtype == F32 and tuple(flat.shape) == (3, 51) and flat.dtype == torch.bool
        assert tuple(ratios.shape) == (3, 3, 2) and ratios.dtype == F32
    with pytest.raises(Exception, match="temporal_embed has 2 frames"):
        make_fx(lambda a, lv, tp: ops.encoder_position_embedding_op([a], lv, tp, None, 10000.0, True, None, None, None),
                tracing_mode="fake")(meta(3, 5, 7, dtype=torch.bool), meta(1, 16), meta(2, 16))


@pytest.mark.parametrize("dynamic", [False, True])
def test_export_gives_one_op_node_for_static_and_dynamic_sizes(dynamic):
    import devis_amd

    class Input(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.level_embed = torch.nn.Parameter(torch.zeros(2, 16, device="meta"))
            self.temporal_embed = torch.nn.Parameter(torch.zeros(3, 16, device="meta"))

        def forward(self, a, b):
            pos, flat, ratios = devis_amd.encoder_position_embedding([a, b], self.level_embed, self.temporal_embed)
            return pos, flat, ratios, devis_amd.sine_position_embedding(a, num_pos_feats=8, normalize=True)

    args = (torch.empty(3, 5, 7, dtype=torch.bool, device="meta"), torch.empty(3, 3, 4, dtype=torch.bool, device="meta"))
    shapes = ({2: torch.export.Dim("W", min=2, max=4096)}, None) if dynamic else None
    graph = torch.export.export(Input(), args, dynamic_shapes=shapes).graph
    node, = _nodes(graph, "encoder_position_embedding")
    sine, = _nodes(graph, "sine_position_embedding")
    pos, flat, ratios = node.meta["val"]
    assert len(pos.shape) == 3 and pos.shape[0] == 3 and pos.shape[2] == 16 and tuple(ratios.shape) == (3, 2, 2)
    assert flat.dtype == torch.bool and tuple(sine.meta["val"].shape[:3]) == (3, 16, 5)
    assert not isinstance(pos.shape[1], int) if dynamic else tuple(pos.shape) == (3, 47, 16)


# ---- documents ---------------------------------------------------------------------------------------------------------------

def test_the_documents_describe_the_operator():
    import devis_amd
    read = lambda name: open(os.path.join(ROOT, name)).read()      # noqa: E731
    design, integration, readme = read("DESIGN.md"), read("INTEGRATION.md"), read("README.md")
    assert re.search(r"^## 18\. .*position", design, re.M | re.I) and "estimate" in design.split("## 18.")[1]
    for out_of_scope in ("PositionEmbeddingSpatialTemporalSine", "src + pos", "Swin"):
        assert out_of_scope in design, out_of_scope
    assert re.search(r"^#+ Encoder input: position", integration, re.M) and "patch_position_encoding" in integration
    assert "patch_transformer" in integration.split("Encoder input: position")[1]
    assert "encoder_position_embedding" in readme and "posembed.h" in readme
    assert "posembed.h" in devis_amd.__doc__ and "encoder_position_embedding" in devis_amd.__doc__
    assert os.path.exists(os.path.join(ROOT, "scripts", "posembed_bench.py"))
    if not os.path.exists(os.path.join(ROOT, "profiles", "posembed_bench.json")):
        assert "no ratio is quoted" in readme
