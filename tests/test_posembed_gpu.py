"""GPU tests of the encoder's positional input (include/posembed.h) against the float64 oracle of tests/posembed_oracle.py and
the reference fixtures.

Exact results: the counts, mask_flatten and valid_ratios are compared with ``==`` against torch on the same masks, on the
device.  There torch divides a tensor by a host scalar by multiplying with the scalar's float32 reciprocal, and so do the
kernels; the CPU, where the fixtures and the oracle's valid ratios were computed, divides.  A product of two correctly rounded
factors lies within 1.5 ulp of the true quotient and the correctly rounded quotient within 0.5, so against CPU values the
valid ratios (at most 1) are held to 2 ulp of a number below 1: ``RATIO_ULPS`` = 2^-23.

Float32 parity: the embedding is held to the float64 oracle within ``min(1e-4, 4 * d + 1e-6)``, where ``d`` is the largest
deviation of the float32 YARDSTICK -- the stock formulation (posembed_oracle in float32) run on the CPU -- from the same
oracle on that case: the kernels may use a different, equally accurate sinf, and are allowed four times the stock
formulation's own error; 1e-4 is the project's float32 parity limit.  Each test prints the measured deviation and the bound
and carries them in its assertion message.

16-bit outputs are compared bit for bit: with the operator's own float32 result rounded once, and with ``round_dtype`` with
the oracle's two-rounding arithmetic applied to the operator's float32 sine values.

Backward: the gradients the parity test uses are multiples of 1/8 in [-2, 2], so every float32 sum of them is exact in any
order: the float32 yardstick (autograd of the oracle in float32 on the CPU) does not deviate from the float64 oracle at all,
the bound of the same kind is ``4 * 0 + 1e-6``, and the segmentation and indexing are checked exactly (three frames of at
most 2015 tokens: the largest sum stays below 2^24 / 8).  The backward cases cover one and several channel blocks of both
passes -- 64 channels per workgroup in the partial pass, 256 in the combine pass -- and the largest number of levels.
Rounding and order are what the bitwise tests are for: with normal random gradients two runs, and a call with the levels
permuted, give the same bits, within the project's 1e-4 (relative to the largest gradient) of the oracle."""
import pytest
import torch

import posembed_oracle
from test_posembed_cpu import (RESULTS, SIZES, check_six, load_fixture, nested, prepare_inputs, reference_modules,
                               stand_in_model)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
PYRAMID = [(23, 37), (12, 19), (6, 10), (3, 5)]
RATIO_ULPS = 2.0 ** -23
# name -> (N, sizes, C, normalize, temporal_embed present)
CASES = {
    "1x1": (2, [(1, 1)], 4, True, True),
    "3x70": (2, [(3, 70)], 8, True, False),             # a row prefix across one 64-pixel chunk boundary
    "2x130": (2, [(2, 130)], 8, True, True),            # ... and across two
    "5x7": (3, [(5, 7)], 16, True, True),
    "5x7-c12": (3, [(5, 7)], 12, True, True),           # N * S * C = 1260: a tail of 4 elements for the 16-bit outputs
    "5x7-c256": (3, [(5, 7)], 256, True, True),
    "23x37": (3, [(23, 37)], 16, True, False),
    "23x37-plain": (3, [(23, 37)], 16, False, True),    # unnormalised: arguments up to 37
    "pyramid": (3, PYRAMID, 16, True, True),            # four levels of unequal size
    "3x300": (2, [(3, 300)], 8, True, True),            # two column jobs of the counts pass, the second ragged; five chunks a row
    "2x257": (2, [(2, 257)], 8, True, False),           # the second column job has one lane
    # POSEMBED_MAX_LEVELS levels: three of equal area, two of those identical
    "levels8": (3, [(6, 9), (4, 7), (3, 4), (4, 3), (3, 4), (2, 2), (1, 5), (1, 1)], 8, True, True),
}


def make_masks(name):
    """bool masks [N, H, W] per level on the CPU: frame 0 has a rectangular padding, frame 1 random holes and, where there
    is room, a fully masked column and row, the last of three frames is fully masked."""
    N, sizes = CASES[name][:2]
    g = torch.Generator().manual_seed(sum(ord(c) for c in name))
    masks = []
    for h, w in sizes:
        m = torch.zeros(N, h, w, dtype=torch.bool)
        if h > 1 and w > 1:
            m[0, h - max(1, h // 3):, :] = True
            m[0, :, w - max(1, w // 4):] = True
        m[1] = torch.rand(h, w, generator=g) < 0.3
        if h > 2 and w > 3:
            m[1, :, 2] = True
            m[1, 1, :] = True
        if N > 2:
            m[2] = True
        masks.append(m)
    return masks


_REFERENCE = {}


def reference(name):
    """Of a case, computed once, shared, read only: the masks, the embeddings, the float64 oracle's three results, and the
    float32 yardstick's deviation from the oracle with the bound it gives."""
    if name not in _REFERENCE:
        N, sizes, C, normalize, with_temporal = CASES[name]
        g = torch.Generator().manual_seed(len(name) + C)
        masks = make_masks(name)
        level = torch.randn(len(sizes), C, generator=g)
        temporal = torch.randn(N, C, generator=g) if with_temporal else None
        wide = None if temporal is None else temporal.double()
        oracle = posembed_oracle.encoder(masks, level.double(), wide, normalize=normalize)
        yardstick = posembed_oracle.encoder(masks, level, temporal, normalize=normalize, dtype=F32)[0]
        deviation = float((yardstick.double() - oracle[0]).abs().max())
        _REFERENCE[name] = dict(masks=masks, level=level, temporal=temporal, oracle=oracle, deviation=deviation,
                                bound=min(1e-4, 4 * deviation + 1e-6), normalize=normalize, sizes=sizes, C=C, N=N)
    return _REFERENCE[name]


def on_device(r):
    return ([m.to(DEV) for m in r["masks"]], r["level"].to(DEV), None if r["temporal"] is None else r["temporal"].to(DEV))


def run(r, **kw):
    import devis_amd
    masks, level, temporal = on_device(r)
    return devis_amd.encoder_position_embedding(masks, level, temporal, normalize=r["normalize"], **kw)


def assert_parity(got, want, r, what):
    err = float((got.detach().double().cpu() - want).abs().max())
    message = "%s: error %.3e; the float32 yardstick deviates by %.3e, bound %.3e" % (what, err, r["deviation"], r["bound"])
    print(message)
    assert got.shape == want.shape and not bool(torch.isnan(got).any()) and err <= r["bound"], message


# ---- exact results -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_counts_masks_and_valid_ratios_are_exact(name):
    from devis_amd.functions import position_embedding as P
    r = reference(name)
    masks = on_device(r)[0]
    cy, cx, ty, tx, mask_flatten, valid_ratios = P.counts(masks)
    want = [posembed_oracle.counts(m) for m in masks]                  # torch's cumsum on the same device tensors
    N = r["N"]
    for got, k in ((cy, 0), (cx, 1), (ty, 2), (tx, 3)):
        assert got.dtype == torch.int32
        assert torch.equal(got.long(), torch.cat([w[k].reshape(N, -1) for w in want], 1)), (name, k)
    assert mask_flatten.dtype == torch.bool and torch.equal(mask_flatten, torch.cat([m.flatten(1) for m in masks], 1))
    assert valid_ratios.dtype == F32 and torch.equal(valid_ratios, torch.stack([posembed_oracle.valid_ratio(m) for m in masks], 1))
    assert float((valid_ratios.cpu() - r["oracle"][2]).abs().max()) <= RATIO_ULPS and torch.equal(mask_flatten.cpu(), r["oracle"][1])


# ---- float32 parity, and the two layouts ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_float32_embedding_is_within_the_yardsticks_error_of_the_oracle(name):
    r = reference(name)
    pos, mask_flatten, valid_ratios = run(r)
    assert pos.dtype == F32 and not pos.requires_grad
    assert_parity(pos, r["oracle"][0], r, name)
    assert torch.equal(mask_flatten.cpu(), r["oracle"][1]) and float((valid_ratios.cpu() - r["oracle"][2]).abs().max()) <= RATIO_ULPS


@pytest.mark.parametrize("name", ["1x1", "2x130", "5x7-c12", "23x37-plain", "pyramid", "levels8"])
def test_both_layouts_agree(name):
    import devis_amd
    r = reference(name)
    masks, level, _ = on_device(r)
    flat = devis_amd.encoder_position_embedding(masks, torch.zeros_like(level), None, normalize=r["normalize"])[0]
    at = 0
    for m, (h, w) in zip(masks, r["sizes"]):
        nchw = devis_amd.sine_position_embedding(m, num_pos_feats=r["C"] // 2, normalize=r["normalize"])
        assert tuple(nchw.shape) == (r["N"], r["C"], h, w) and nchw.dtype == F32
        assert torch.equal(nchw.flatten(2).transpose(1, 2), flat[:, at:at + h * w]), (name, h, w)
        want = posembed_oracle.sine(m.cpu(), r["C"] // 2, normalize=r["normalize"])
        err = float((nchw.double().cpu() - want).abs().max())
        assert err <= r["bound"], "%s %dx%d: error %.3e, bound %.3e" % (name, h, w, err, r["bound"])
        at += h * w


def test_other_settings_and_non_contiguous_masks():
    import devis_amd
    r = reference("pyramid")
    masks, level, temporal = on_device(r)
    want = run(r)
    # the same values from masks that are views: transposed storage, every other row of a taller tensor, an expanded frame
    views = [masks[0].transpose(1, 2).contiguous().transpose(1, 2),
             torch.stack([masks[1], ~masks[1]], 2).flatten(1, 2)[:, ::2],
             masks[2], masks[3].unsqueeze(1).expand(-1, 2, -1, -1)[:, 1]]
    assert not views[0].is_contiguous() and not views[1].is_contiguous() and all(torch.equal(v, m) for v, m in zip(views, masks))
    for g, w in zip(devis_amd.encoder_position_embedding(views, level, temporal), want):
        assert torch.equal(g, w)
    fully = torch.zeros(2, 4, 6, dtype=torch.bool, device=DEV).expand(2, 4, 6)[:1].expand(2, 4, 6)          # stride 0 over frames
    assert torch.equal(devis_amd.sine_position_embedding(fully, num_pos_feats=4)[0], devis_amd.sine_position_embedding(fully, num_pos_feats=4)[1])
    # temperature and scale
    m = r["masks"][0]
    for kw in (dict(temperature=20, normalize=True, scale=3.0), dict(temperature=10000, normalize=False)):
        oracle = posembed_oracle.sine(m, 8, **kw)
        deviation = float((posembed_oracle.sine(m, 8, dtype=F32, **kw).double() - oracle).abs().max())
        got = devis_amd.sine_position_embedding(masks[0], num_pos_feats=8, **kw)
        err = float((got.double().cpu() - oracle).abs().max())
        assert err <= min(1e-4, 4 * deviation + 1e-6), "%s: error %.3e, yardstick %.3e" % (kw, err, deviation)


# ---- 16-bit outputs ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", ["5x7-c12", "pyramid", "1x1", "levels8"])
def test_16_bit_outputs_are_the_float32_result_rounded_once(name, dtype):
    import devis_amd
    r = reference(name)
    masks, level, temporal = on_device(r)
    full = run(r)[0]
    assert torch.equal(run(r, out_dtype=dtype)[0], full.to(dtype))
    nchw = devis_amd.sine_position_embedding(masks[0], num_pos_feats=r["C"] // 2, normalize=r["normalize"])
    assert torch.equal(devis_amd.sine_position_embedding(masks[0], num_pos_feats=r["C"] // 2, normalize=r["normalize"], out_dtype=dtype),
                       nchw.to(dtype))
    # with round_dtype: the two roundings of `.to(dtype)` followed by `+ level_embed`, on the operator's own sine values
    sine = devis_amd.encoder_position_embedding(masks, torch.zeros_like(level), None, normalize=r["normalize"])[0]
    for out_dtype, level_dtype in ((F32, F32), (dtype, dtype), (dtype, F32)):
        got = devis_amd.encoder_position_embedding(masks, level.to(level_dtype), temporal, normalize=r["normalize"], round_dtype=dtype,
                                                   out_dtype=None if out_dtype == torch.promote_types(dtype, level_dtype) else out_dtype)[0]
        want = posembed_oracle.embed_rounded(sine, r["sizes"], level.to(level_dtype), temporal, dtype, out_dtype)
        assert got.dtype == out_dtype and torch.equal(got, want), (name, dtype, out_dtype, level_dtype)


# ---- backward ----------------------------------------------------------------------------------------------------------------

# name -> (sizes, C); N = 3.  The partial pass covers 64 channels per workgroup, the combine pass 256.
BACKWARD = {
    "pyramid": (PYRAMID, 8), "chunks": ([(40, 50), (3, 5)], 8), "5x7": ([(5, 7)], 8),
    "c72": ([(40, 50), (3, 5)], 72),                    # two channel blocks in the partial pass, the second with 8 live lanes
    "c260": ([(5, 7), (3, 5)], 260),                    # five of them, and two in the combine pass, the second ragged
    "c256": (PYRAMID, 256),                             # the model's width
    "levels8": (CASES["levels8"][1], 8),
}


def backward_case(name, exact):
    sizes, C = BACKWARD[name]
    g = torch.Generator().manual_seed(len(name))
    masks = [torch.rand(3, h, w, generator=g) < 0.3 for h, w in sizes]
    S = sum(h * w for h, w in sizes)
    grad = torch.randint(-16, 17, (3, S, C), generator=g).float() / 8 if exact else torch.randn(3, S, C, generator=g)
    return masks, torch.randn(len(sizes), C, generator=g), torch.randn(3, C, generator=g), grad


def gradients(masks, level, temporal, grad, want=(True, True), **kw):
    import devis_amd
    level = level.to(DEV).requires_grad_(want[0])
    temporal = temporal.to(DEV).requires_grad_(want[1])
    pos = devis_amd.encoder_position_embedding([m.to(DEV) for m in masks], level, temporal, **kw)[0]
    assert pos.requires_grad
    pos.backward(grad.to(DEV).to(pos.dtype))
    return level.grad, temporal.grad


@pytest.mark.parametrize("name", list(BACKWARD))
def test_backward_equals_autograd_of_the_oracle(name):
    from devis_amd import _posembed
    masks, level, temporal, grad = backward_case(name, exact=True)
    if name == "chunks":
        assert 40 * 50 > 3 * _posembed.tile(_posembed.TILE_TOKENS)         # a segment of several chunks
    per_block = _posembed.tile(_posembed.TILE_CHANNELS)
    assert {"c72": 2, "c260": 5, "c256": 4}.get(name, 1) == -(-BACKWARD[name][1] // per_block)      # channel blocks of the partial pass
    lv, tp = level.double().requires_grad_(True), temporal.double().requires_grad_(True)
    posembed_oracle.encoder(masks, lv, tp)[0].backward(grad.double())
    lv32, tp32 = level.clone().requires_grad_(True), temporal.clone().requires_grad_(True)
    posembed_oracle.encoder(masks, lv32, tp32, dtype=F32)[0].backward(grad)
    deviation = max(float((lv32.grad.double() - lv.grad).abs().max()), float((tp32.grad.double() - tp.grad).abs().max()))
    bound = min(1e-4, 4 * deviation + 1e-6)
    got = gradients(masks, level, temporal, grad)
    for g, w, what in ((got[0], lv.grad, "grad_level_embed"), (got[1], tp.grad, "grad_temporal_embed")):
        err = float((g.double().cpu() - w).abs().max())
        message = "%s %s: error %.3e; the float32 yardstick deviates by %.3e, bound %.3e" % (name, what, err, deviation, bound)
        print(message)
        assert g.dtype == F32 and g.shape == w.shape and err <= bound, message
    # 16-bit gradients of pos, and 16-bit embeddings: the same sums (multiples of 1/8 are exact there too)
    half = gradients(masks, level.half(), temporal.half(), grad, round_dtype=torch.float16)
    assert half[0].dtype == torch.float16 and torch.equal(half[0].double().cpu(), lv.grad.half().double())
    assert torch.equal(half[1].double().cpu(), tp.grad.half().double())


def test_gradients_are_bitwise_reproducible_and_do_not_depend_on_the_order_of_the_levels():
    masks, level, temporal, grad = backward_case("pyramid", exact=False)
    first = gradients(masks, level, temporal, grad)
    again = gradients(masks, level, temporal, grad)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    want = posembed_oracle.embedding_gradients(grad.double(), PYRAMID)
    for g, w in zip(first, want):
        assert float((g.double().cpu() - w).abs().max()) <= 1e-4 * max(1.0, float(w.abs().max()))
    perm, at, starts = [2, 0, 3, 1], 0, []
    for h, w in PYRAMID:
        starts.append(at)
        at += h * w
    moved = torch.cat([grad[:, starts[l]:starts[l] + PYRAMID[l][0] * PYRAMID[l][1]] for l in perm], 1)
    other = gradients([masks[l] for l in perm], level[perm], temporal, moved)
    assert torch.equal(other[0], first[0][perm]) and torch.equal(other[1], first[1])


def test_only_the_requested_gradient_is_computed(monkeypatch):
    only_the_requested_gradient("5x7", monkeypatch)


def test_only_the_requested_gradient_is_computed_with_two_channel_blocks(monkeypatch):
    only_the_requested_gradient("c72", monkeypatch)         # both null-pointer branches of the combine pass, C > 64


def only_the_requested_gradient(name, monkeypatch):
    from devis_amd import _posembed
    masks, level, temporal, grad = backward_case(name, exact=True)
    both = gradients(masks, level, temporal, grad)
    seen, real = [], _posembed.backward
    monkeypatch.setattr(_posembed, "backward", lambda code, g, shape, ws, gl, gt: seen.append((gl is not None, gt is not None)) or real(code, g, shape, ws, gl, gt))
    only_level = gradients(masks, level, temporal, grad, want=(True, False))
    only_temporal = gradients(masks, level, temporal, grad, want=(False, True))
    assert seen == [(True, False), (False, True)]
    assert only_level[1] is None and torch.equal(only_level[0], both[0])
    assert only_temporal[0] is None and torch.equal(only_temporal[1], both[1])
    import devis_amd
    pos = devis_amd.encoder_position_embedding([m.to(DEV) for m in masks], level.to(DEV), temporal.to(DEV))[0]
    assert not pos.requires_grad and len(seen) == 2


# ---- the drop-in modules and the patched prepare_data ------------------------------------------------------------------------

def fixture_bound(d, key, oracle):
    deviation = float((d[key].double() - oracle).abs().max())
    return deviation, min(1e-4, 4 * deviation + 1e-6)


def test_modules_give_the_reference_tensors():
    from devis_amd import modules
    s = load_fixture("posembed_sine")
    mask = s["mask"].to(DEV)
    for key, args, kw in (("pos_plain", (8,), {}), ("pos_normalized", (8, 10000, True), dict(normalize=True)),
                          ("pos_scaled", (8, 20, True, 3.0), dict(temperature=20, normalize=True, scale=3.0))):
        oracle = posembed_oracle.sine(s["mask"], 8, **kw)
        deviation, bound = fixture_bound(s, key, oracle)
        got = modules.PositionEmbeddingSine(*args).to(DEV)(nested(mask))
        err = float((got.double().cpu() - oracle).abs().max())
        assert got.dtype == F32 and err <= bound, "%s: error %.3e; the reference deviates by %.3e, bound %.3e" % (key, err, deviation, bound)
    t = load_fixture("posembed_temporal")
    module = modules.PositionEmbeddingSineWithLearnableTemporal(16, num_frames=3, normalize=True)
    module.load_state_dict({"temporal_embed": t["temporal_embed"]})
    module = module.to(DEV)
    oracle = posembed_oracle.sine(t["mask"], 8, normalize=True) + t["temporal_embed"].double()[:, :, None, None]
    deviation, bound = fixture_bound(t, "pos", oracle)
    got = module(nested(t["mask"].to(DEV)))
    err = float((got.detach().double().cpu() - oracle).abs().max())
    assert err <= bound, "temporal: error %.3e; the reference deviates by %.3e, bound %.3e" % (err, deviation, bound)
    got.sum().backward()
    assert torch.equal(module.temporal_embed.grad.cpu(), torch.full((3, 16), 35.0))


@pytest.mark.parametrize("transformer_first", [True, False])
def test_patched_prepare_data_gives_the_six_results_with_one_fused_call(transformer_first, monkeypatch):
    import devis_amd
    from devis_amd import ops
    d = load_fixture("posembed_prepare")
    _, masks_cpu, level_embed, temporal_embed = prepare_inputs(d)
    oracle = posembed_oracle.encoder(masks_cpu, level_embed.double(), temporal_embed.double())[0]
    deviation, bound = fixture_bound(d, "lvl_pos_embed_flatten", oracle)
    calls, real_encoder, real_sine = [], ops.encoder_position_embedding, ops.sine_position_embedding
    monkeypatch.setattr(ops, "encoder_position_embedding", lambda *a, **k: calls.append("encoder") or real_encoder(*a, **k))
    monkeypatch.setattr(ops, "sine_position_embedding", lambda *a, **k: calls.append("sine") or real_sine(*a, **k))
    encoding, transformer = reference_modules()
    pe, top, srcs, masks = stand_in_model(encoding, transformer, d, DEV)
    stock = top.prepare_data(srcs, masks, [pe(nested(m)).to(F32) for m in masks])             # the stock classes on the device
    check_six(stock, d, exact=False, tol=bound)
    undo_t = devis_amd.patch_transformer(transformer) if transformer_first else None
    undo = devis_amd.patch_position_encoding(encoding, transformer)
    if not transformer_first:
        undo_t = devis_amd.patch_transformer(transformer)
    try:
        got = top.prepare_data(srcs, masks, [pe(nested(m)).to(F32) for m in masks])
        assert calls == (["encoder"] if transformer_first else ["sine"] * 3)                   # the documented order fuses
        err = float((got[2].detach().double().cpu() - oracle).abs().max())
        message = "error %.3e; the reference deviates by %.3e, bound %.3e" % (err, deviation, bound)
        print(message)
        assert err <= bound, message
        check_six(got, d, exact=False, tol=2 * bound)
        assert torch.equal(got[5], stock[5]) and torch.equal(got[1], stock[1]) and torch.equal(got[0], stock[0])       # torch's, on the device
        assert got[3] is devis_amd.argument_builders.interned_pyramid(SIZES, DEV)[0]
        assert [r.dtype for r in got] == [d[k].dtype for k in RESULTS]
        g = torch.randint(-16, 17, got[2].shape, device=DEV).float() / 8
        got[2].backward(g)
        want = posembed_oracle.embedding_gradients(g.double().cpu(), SIZES)
        assert torch.equal(top.level_embed.grad.double().cpu(), want[0]) and torch.equal(pe.temporal_embed.grad.double().cpu(), want[1])
        # autocast-like use: `.to(bfloat16)` of the caller is the operator's round_dtype
        del calls[:]
        low = top.prepare_data(srcs, masks, [pe(nested(m)).to(torch.bfloat16) for m in masks])[2]
        want_low = torch.cat([(posembed_oracle.sine(m, 8, normalize=True, dtype=F32) + pe.temporal_embed.detach()[:, :, None, None])
                              .to(torch.bfloat16).flatten(2).transpose(1, 2) + top.level_embed.detach()[l] for l, m in enumerate(masks)], 1)
        assert low.dtype == F32 and float((low.detach() - want_low).abs().max()) <= 2.0 ** -8 * 8       # an ulp of bfloat16 below 8
    finally:
        if not transformer_first:
            devis_amd.argument_builders.unpatch_transformer(transformer, undo_t)
        devis_amd.unpatch_position_encoding(encoding, transformer, undo)
        if transformer_first:
            devis_amd.argument_builders.unpatch_transformer(transformer, undo_t)
