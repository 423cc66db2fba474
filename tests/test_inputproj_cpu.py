"""CPU tests of the encoder's input projections (include/inputproj.h): the torch composite of
``devis_amd.group_norm_tokens`` against the float64 oracle, the conditioning of every case the GPU file uses, argument errors,
the routing predicate, the deferred object, patching and unpatching, the shared ``src_flatten`` helper, and the patched stand-in
model against the fixture recorded from the reference.  No GPU is needed: on CPU tensors the operator is its composite.
"""
import pytest
import torch

import inputproj_cases as K
import inputproj_oracle as O
from inputproj_cases import BF16, F16, F32

GRADS = ("grad_x", "grad_weight", "grad_bias")


def op():
    import devis_amd
    return devis_amd.group_norm_tokens


def worst(got, want, gradients=True):
    devs = [K.deviation(got["tokens"], want["tokens"])]
    if gradients:
        devs += [K.deviation(g, w) for name in GRADS for g, w in zip(got[name], want[name])]
    return max(devs)


def test_float64_composite_equals_the_oracle():
    from devis_amd.functions.input_projection import group_norm_tokens_composite
    for shape in K.SHAPES[:9]:
        for N, C, G, levels, mean, gradients in K.oracle_checks(shape):
            d, want = K.case(N, C, G, levels, mean)
            d64 = {k: ([t.double() for t in v] if isinstance(v, list) else v.double() if isinstance(v, torch.Tensor) else v)
                   for k, v in d.items()}
            for fn in (group_norm_tokens_composite, op()):              # (on the CPU the operator is the composite)
                assert worst(K.run(d64, fn), want, gradients) <= 1e-10, (N, C, G, levels, mean)


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "%dx%d-%s" % (s[0] + ("+".join("%dx%d" % hw for hw in s[1]),)))
def test_every_case_of_the_gpu_tests_is_well_conditioned(shape):
    """Plain float32 torch stays within 1e-5 of the oracle -- a tenth of the float32 bar -- on every case of
    tests/test_inputproj_gpu.py with the tests' own seeds: an ill-conditioned draw cannot hide behind the bar."""
    from devis_amd.functions.input_projection import group_norm_tokens_composite
    for N, C, G, levels, mean, gradients in K.oracle_checks(shape):
        d, want = K.case(N, C, G, levels, mean)
        assert not gradients or K.min_group(C, G, levels) >= 4
        assert worst(K.run(d, group_norm_tokens_composite), want, gradients) <= 1e-5, (N, C, G, levels, mean)


def test_the_other_gpu_cases_are_well_conditioned():
    from devis_amd.functions.input_projection import group_norm_tokens_composite
    import test_inputproj_gpu as T
    cases = [T.FOUR + (4.0,), T.TAILS + (4.0,), (1, 260, 4, ((19, 27), (1, 1)), 0.0), (3, 256, 32, K.PYRAMID, 0.0),
             (2, 12, 4, K.PYRAMID[:3], 4.0), (1, 256, 32, ((19, 27),), 0.0)]
    for N, C, G, levels, mean in cases:
        d, want = K.case(N, C, G, levels, mean)
        assert K.min_group(C, G, levels) >= 4
        assert worst(K.run(d, group_norm_tokens_composite), want) <= 1e-5, (N, C, G, levels, mean)


def test_oracle_statistics_are_those_of_a_contiguous_run():
    x = K.rand(2, 6, 3, 4, seed=1, shift=4.0)
    mean, rstd = O.statistics([x], 3)
    runs = x.double().reshape(2, 3, 24)
    assert torch.allclose(mean[:, 0], runs.mean(2), rtol=0, atol=1e-12)
    assert torch.allclose(rstd[:, 0], 1 / torch.sqrt(runs.var(2, unbiased=False) + 1e-5), rtol=0, atol=1e-12)


def test_argument_errors():
    x, w, b = torch.randn(2, 8, 3, 4), torch.ones(8), torch.zeros(8)
    bad = [
        (([], 4, [], []), "one weight and one bias per map"),
        (([x], 4, [w, w], [b]), "one weight and one bias per map"),
        (([x[0]], 4, [w], [b]), r"must be \[N, C, H, W\]"),
        (([x], 3, [w], [b]), "multiple of num_groups"),
        (([x], 0, [w], [b]), "multiple of num_groups"),
        (([x, torch.randn(2, 4, 3, 4)], 4, [w, w], [b, b]), "map 1 must be"),
        (([x, torch.randn(3, 8, 3, 4)], 4, [w, w], [b, b]), "map 1 must be"),
        (([x, x.double()], 4, [w, w], [b, b]), "map 1 must be"),
        (([x], 4, [torch.ones(4)], [b]), "weight 0 must be"),
        (([x], 4, [w], [b.double()]), "bias 0 must be"),
        (([x], 4, [w], [None]), "bias 0 must be"),
    ]
    for args, message in bad:
        with pytest.raises(RuntimeError, match=message):
            op()(*args)


def test_binding_reports_shapes_limits_and_workspaces_without_a_gpu():
    from devis_amd import _inputproj as B
    assert B.tile(B.TILE_MAX_LEVELS) == B.MAX_LEVELS and B.tile(B.TILE_MAX_CHANNELS) == B.MAX_CHANNELS
    chunk, sums = B.tile(B.TILE_STAT_CHUNK), B.tile(B.TILE_SUM_CHUNK)
    assert B.tile(B.TILE_PIXELS) == 64 and B.tile(B.TILE_CHANNELS) == 64 and sums % B.tile(B.TILE_PIXELS) == 0
    shape = B.shape_of(3, 256, 32, K.PYRAMID)
    assert B.tokens(shape) == 52
    assert B.forward_workspace_bytes(shape) == 0                                 # every group is one chunk: no combine launch
    two = B.shape_of(2, 256, 32, [(19, 27)])
    assert 8 * 19 * 27 > chunk and B.forward_workspace_bytes(two) == 2 * 32 * 2 * 2 * 4
    assert B.backward_workspace_bytes(two) == 2 * 2 * 256 * 2 * 4 + 256 * ((2 * 32 * 2 * 4 + 255) // 256)
    for bad in (B.shape_of(1, 2048, 32, [(2, 2)]), B.shape_of(1, 8, 3, [(2, 2)]), B.shape_of(1, 8, 0, [(2, 2)])):
        with pytest.raises(RuntimeError, match="inputproj_tokens failed"):
            B.tokens(bad)
    with pytest.raises(ValueError):
        B.shape_of(1, 8, 4, [(1, 1)] * 9)
    lib = B.load()
    assert all(hasattr(lib, name) for name in B.EXPORTED_SYMBOLS)


def test_routing_predicate(monkeypatch):
    from devis_amd.functions import input_projection as F
    x, w = torch.randn(2, 8, 3, 4), torch.ones(8)
    assert not F.takes_kernels([x], 4, [w])                                      # CPU tensors
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    assert F.takes_kernels([x], 4, [w])
    assert F.takes_kernels([x.bfloat16()], 4, [w], F32) and F.takes_kernels([x.half()], 4, [w.half()])
    assert F.takes_kernels([x], 4, [w], BF16) and F.takes_kernels([x], 4, [w], F16)
    assert not F.takes_kernels([x.double()], 4, [w.double()])                    # float64
    assert not F.takes_kernels([x], 4, [w.bfloat16()])                           # another mix: narrower parameters
    assert not F.takes_kernels([x.bfloat16()], 4, [w.half()]) and not F.takes_kernels([x.bfloat16()], 4, [w], F16)
    assert not F.takes_kernels([x] * 9, 4, [w] * 9)                              # above the limits
    assert F.takes_kernels([x] * 8, 4, [w] * 8)
    assert not F.takes_kernels([torch.randn(1, 1032, 1, 1)], 8, [torch.ones(1032)])
    assert F.takes_kernels([torch.randn(1, 1024, 1, 1)], 8, [torch.ones(1024)])
    assert not F.takes_kernels([x, torch.randn(2, 8, 0, 4)], 4, [w, w])          # no elements
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    assert not F.takes_kernels([x], 4, [w])
    for mix in K.MIXES + [(F32, F32, F32)]:
        assert F.supported(*mix)


def test_empty_maps_take_the_composite():
    x, w, b = torch.randn(2, 8, 0, 4), torch.ones(8), torch.zeros(8)
    assert tuple(op()([x], 4, [w], [b]).shape) == (2, 0, 8)


# ---- the deferred object and the patch ---------------------------------------------------------------------------------------

def small_model(levels=4, channels=(4, 6, 8), hidden=64):
    torch.manual_seed(5)
    model = K.DeformableDETR(list(channels), hidden, levels)
    with torch.no_grad():
        for name, p in model.input_proj.named_parameters():
            if name.endswith("1.weight") or name.endswith("1.bias"):
                p.copy_(torch.randn_like(p) + (1.0 if name.endswith("weight") else 0.0))
    features = [torch.randn(2, c, h, w) for c, (h, w) in zip(channels, K.PYRAMID)]
    return model, features


def test_deferred_object_answers_without_computing_and_materialises_once(monkeypatch):
    import devis_amd
    from devis_amd.modules import input_projection as M
    model, features = small_model()
    calls = []
    monkeypatch.setattr(M, "group_norm_tokens", lambda *a, _f=M.group_norm_tokens: (calls.append(len(a[0])), _f(*a))[1])
    previous = devis_amd.patch_input_proj(model)
    try:
        src = model.input_proj[0](features[0])
    finally:
        devis_amd.unpatch_input_proj(model, previous)
    assert isinstance(src, devis_amd.DeferredInputProjection)
    assert src.shape == torch.Size((2, 64, 5, 7)) and src.dtype == torch.float32 and src.device == features[0].device
    assert calls == []
    want = model.input_proj[0](features[0])
    flat = src.flatten(2)
    assert calls == [1] and torch.allclose(flat, want.flatten(2), rtol=0, atol=1e-5)
    view = src.materialize()
    assert view is src.materialize() and calls == [1]
    assert tuple(view.shape) == (2, 64, 5, 7) and view.stride() == (35 * 64, 1, 7 * 64, 64)        # channels last: a view of the tokens
    assert torch.equal(src * 2.0, view * 2.0) and torch.equal(torch.cat([src, src], 1), torch.cat([view, view], 1))
    assert torch.equal(torch.nn.functional.relu(src), view.relu()) and calls == [1]


def test_patch_and_unpatch_restore_every_attribute():
    import devis_amd
    model, features = small_model()
    before_state = {k: v.clone() for k, v in model.state_dict().items()}
    before = [(type(p[1]), dict(p[1].__dict__)) for p in model.input_proj]
    want = [p(f) for p, f in zip(model.input_proj, features)]
    previous = devis_amd.patch_input_proj(model)
    assert all(type(p[1]) is devis_amd.modules.input_projection.DeferringGroupNorm for p in model.input_proj)
    assert list(model.state_dict()) == list(before_state)
    devis_amd.unpatch_input_proj(model, previous)
    assert [(type(p[1]), dict(p[1].__dict__)) for p in model.input_proj] == before
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), before_state.values()))
    assert all(torch.equal(p(f), w) for p, f, w in zip(model.input_proj, features, want))


def test_a_projection_that_feeds_the_next_one_is_not_deferred():
    import devis_amd
    model, features = small_model(levels=6)
    model, features = model.double(), [f.double() for f in features]          # (1 x 1 levels: groups of 2 elements, cascaded)
    want, srcs_want, _ = model(features)
    previous = devis_amd.patch_input_proj(model)
    previous_points = devis_amd.patch_transformer(K)
    try:
        assert [p[1].defer_output for p in model.input_proj] == [True, True, True, False, False, True]
        got, srcs, _ = model(features)
    finally:
        devis_amd.argument_builders.unpatch_transformer(K, previous_points)
        devis_amd.unpatch_input_proj(model, previous)
    assert [isinstance(s, devis_amd.DeferredInputProjection) for s in srcs] == [True, True, True, False, False, True]
    assert all(isinstance(s, torch.Tensor) and s.permute(0, 2, 3, 1).is_contiguous() for s in srcs[3:5])   # the view of the level's tokens
    assert torch.allclose(got, want, rtol=0, atol=1e-9)
    for s, w in zip(srcs, srcs_want):
        assert tuple(s.shape) == tuple(w.shape)


def test_helper_is_the_cat_bit_for_bit_for_plain_tensors():
    import types
    from devis_amd import argument_builders as A
    srcs = [torch.randn(2, 16, h, w) for h, w in K.PYRAMID]
    masks = [torch.zeros(2, h, w, dtype=torch.bool) for h, w in K.PYRAMID]
    pos = [torch.randn(2, 16, h, w) for h, w in K.PYRAMID]
    want = torch.cat([s.flatten(2).transpose(1, 2) for s in srcs], 1)
    assert torch.equal(A.flatten_sources(srcs), want)
    top = K.DeformableTransformer(16, 4)
    stock = top.prepare_data(srcs, masks, pos)
    for prepare in (A.prepare_data, A.prepare_data_deferred):
        got = prepare(top, srcs, masks, pos)
        assert torch.equal(got[0], want) and torch.equal(got[0], stock[0])
        assert all(torch.equal(g, s) for g, s in zip(got[1:], stock[1:]))


def test_helper_fuses_deferred_levels_and_materialises_a_mix(monkeypatch):
    import devis_amd
    from devis_amd.modules import input_projection as M
    model, features = small_model()
    want = torch.cat([p(f).flatten(2).transpose(1, 2) for p, f in zip(model.input_proj, features)], 1)
    calls = []
    monkeypatch.setattr(M, "group_norm_tokens", lambda *a, _f=M.group_norm_tokens: (calls.append(len(a[0])), _f(*a))[1])
    previous = devis_amd.patch_input_proj(model)
    try:
        srcs = [p(f) for p, f in zip(model.input_proj, features)]
        tokens = devis_amd.argument_builders.flatten_sources(srcs)
        assert calls == [3] and torch.allclose(tokens, want, rtol=0, atol=1e-5)
        start = 0
        for s in srcs:                                                          # bound to views of the one result
            view = s.materialize()
            assert view.data_ptr() == tokens.data_ptr() + start * 64 * 4 and calls == [3]
            start += view.shape[2] * view.shape[3]
        mixed = [model.input_proj[0](features[0]), want.new_zeros(2, 64, 3, 4), model.input_proj[2](features[2])]
        del calls[:]
        tokens = devis_amd.argument_builders.flatten_sources(mixed)
        assert calls == [1, 1] and torch.allclose(tokens[:, :35], want[:, :35], rtol=0, atol=1e-5) and not tokens[:, 35:47].any()
    finally:
        devis_amd.unpatch_input_proj(model, previous)


@pytest.mark.parametrize("fused", [True, False], ids=["patched-prepare-data", "stock-prepare-data"])
def test_patched_model_reproduces_the_fixture_on_the_cpu(fused):
    import devis_amd
    fixture = K.load_fixture()
    model, features = K.build_model(fixture, torch.float64, "cpu")
    previous = devis_amd.patch_input_proj(model)
    previous_points = devis_amd.patch_transformer(K) if fused else None
    try:
        got, srcs, src_flatten = K.run_model(model, features, fixture)
    finally:
        if fused:
            devis_amd.argument_builders.unpatch_transformer(K, previous_points)
        devis_amd.unpatch_input_proj(model, previous)
    assert all(isinstance(s, devis_amd.DeferredInputProjection) for s in srcs)
    for name, want in K.expected(fixture).items():
        err, ref = float((got[name].double() - want.double()).abs().max()), float(want.abs().max())
        assert err <= 1e-6 * ref, (name, err, ref)                             # (the fixture holds float64 results rounded to float32)
