"""GPU tests of the encoder's input projections (include/inputproj.h): ``devis_amd.group_norm_tokens``
against the float64 oracle restated from the header (tests/inputproj_oracle.py), its bitwise properties, results allocated over
stale memory, and the patched stand-in model against the fixture recorded from the reference.

The bars are the project's (tests/test_attmap_gpu.py::assert_close): ``max|got - want| <= tol * max|want|`` per tensor with
``tol = 1e-4`` for a float32 result and ``1e-2`` for a 16-bit one.  No group of fewer than 4 elements is in a gradient test: plain
float32 torch in this formulation, measured on the CPU against float64, deviates by at most 1.7e-6 at the shapes below but by
2e-4 to 1.9e-3 with a 2-element group, and without bound with a 1-element group (variance 0).
tests/test_inputproj_cpu.py asserts that the float32 composite stays within 1e-5 of the oracle on every case used here.
"""
import pytest
import torch

import inputproj_cases as K
import stale_memory
from inputproj_cases import BF16, F16, F32
from test_attmap_gpu import TOL, assert_close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
GRADS = ("grad_x", "grad_weight", "grad_bias")
FOUR = (3, 256, 32, K.PYRAMID)          # the configuration's case of the bitwise tests
TAILS = (2, 12, 4, ((9, 130), (3, 4)))  # per-element stores, pixel-tile tails and several chunks


def op():
    import devis_amd
    return devis_amd.group_norm_tokens


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def all_same_bits(got, want):
    if not same_bits(got["tokens"], want["tokens"]):
        return False
    return all((g is None and w is None) or (g is not None and w is not None and same_bits(g, w))
               for name in GRADS for g, w in zip(got[name], want[name]))


def shifted(t, nbytes=4):
    """A dense view with t's values whose first element is ``nbytes`` bytes past a 256-byte boundary."""
    elements = nbytes // t.element_size()
    base = torch.empty(t.numel() + 256, dtype=t.dtype, device=t.device)
    view = base[elements:elements + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def on_gpu(d):
    return {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def check(N, C, G, levels, mean=0.0, mix=(F32, F32, F32), gradients=True):
    d, want = K.case(N, C, G, levels, mean, mix)
    assert not gradients or K.min_group(C, G, levels) >= 4
    got = K.run(on_gpu(d), op(), out_dtype=mix[2]) if gradients else \
        {"tokens": op()(*(on_gpu(d)[k] for k in ("xs", "num_groups", "weights", "biases")), out_dtype=mix[2])}
    what = "%s mean %g %s" % ((N, C, G, levels), mean, mix)
    assert got["tokens"].dtype == mix[2] and got["tokens"].is_contiguous() and got["tokens"].shape == want["tokens"].shape
    assert_close(got["tokens"], want["tokens"], TOL[mix[2]], what + " tokens")
    if not gradients:
        return
    for name, dt in zip(GRADS, (mix[0], mix[1], mix[1])):
        for l, (g, w) in enumerate(zip(got[name], want[name])):
            assert g.dtype == dt and g.is_contiguous() and g.shape == w.shape
            assert_close(g, w, TOL[dt], "%s %s %d" % (what, name, l))


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "%dx%d-%s" % (s[0] + ("+".join("%dx%d" % hw for hw in s[1]),)))
def test_operator_matches_the_oracle(shape):
    # a level whose groups have fewer than 4 elements is in the forward test only (module docstring; K.oracle_checks)
    for N, C, G, levels, mean, gradients in K.oracle_checks(shape):
        check(N, C, G, levels, mean, gradients=gradients)


@pytest.mark.parametrize("mix", K.MIXES, ids=lambda m: "-".join(str(t).split(".")[1] for t in m))
def test_operator_in_every_accepted_dtype_mix(mix):
    check(3, 256, 32, K.PYRAMID, 0.0, mix)
    check(2, 12, 4, K.PYRAMID[:3], 4.0, mix)
    check(1, 256, 32, ((19, 27),), 0.0, mix)


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_a_group_without_variance_gives_the_bias_bit_for_bit(dtype):
    d, _ = K.case(3, 6, 6, ((1, 1),), 4.0)
    d = on_gpu(d)
    tokens = op()(d["xs"], 6, d["weights"], d["biases"], out_dtype=dtype)
    assert same_bits(tokens, d["biases"][0].to(dtype).expand(3, 1, 6))


@pytest.mark.parametrize("mix", [(F32, F32, F32), (BF16, F32, F32)], ids=["float32", "autocast"])
def test_bits_do_not_depend_on_batch_levels_layout_or_alignment(mix):
    for N, C, G, levels in (FOUR, TAILS):
        d = on_gpu(K.case(N, C, G, levels, 4.0, mix)[0])
        full = K.run(d, op(), out_dtype=mix[2])
        assert all_same_bits(K.run(d, op(), out_dtype=mix[2]), full)                               # two runs
        with torch.no_grad():                                                                      # the route without autograd
            assert same_bits(op()(d["xs"], G, d["weights"], d["biases"], out_dtype=mix[2]), full["tokens"])
        for n in range(N):                                                                          # a frame alone
            one = dict(d, xs=[x[n:n + 1].clone() for x in d["xs"]], grad_tokens=d["grad_tokens"][n:n + 1].clone())
            got = K.run(one, op(), out_dtype=mix[2])
            assert same_bits(got["tokens"], full["tokens"][n:n + 1]), n
            assert all(same_bits(g, f[n:n + 1]) for g, f in zip(got["grad_x"], full["grad_x"])), n
        start = 0
        for l, (h, w) in enumerate(levels):                                                         # a level alone
            one = {"xs": d["xs"][l:l + 1], "weights": d["weights"][l:l + 1], "biases": d["biases"][l:l + 1], "num_groups": G,
                   "grad_tokens": d["grad_tokens"][:, start:start + h * w].contiguous()}
            got = K.run(one, op(), out_dtype=mix[2])
            assert same_bits(got["tokens"], full["tokens"][:, start:start + h * w]), l
            assert all_same_bits(got, {"tokens": got["tokens"], **{k: full[k][l:l + 1] for k in GRADS}}), l
            start += h * w
        last = dict(d, xs=[x.contiguous(memory_format=torch.channels_last) for x in d["xs"]])      # channels-last maps
        assert not last["xs"][0].is_contiguous()
        assert all_same_bits(K.run(last, op(), out_dtype=mix[2]), full)
        for names in (("xs",), ("weights", "biases"), ("grad_tokens",), ("xs", "weights", "biases", "grad_tokens")):
            views = {k: (([shifted(t) for t in v] if isinstance(v, list) else shifted(v)) if k in names else v) for k, v in d.items()}
            assert all_same_bits(K.run(views, op(), out_dtype=mix[2]), full), names


def test_only_the_requested_gradients_are_computed(monkeypatch):
    from devis_amd import _inputproj
    N, C, G, levels = FOUR
    d = on_gpu(K.case(N, C, G, levels, 4.0)[0])
    L = len(levels)
    full = K.run(d, op())
    for which in range(3):
        for l in (0, L - 1):
            wants = tuple([k == which and i == l for i in range(L)] for k in range(3))
            got = K.run(d, op(), wants=wants)
            for k, name in enumerate(GRADS):
                for i in range(L):
                    if wants[k][i]:
                        assert same_bits(got[name][i], full[name][i]), (name, i)
                    else:
                        assert got[name][i] is None
    calls = []
    monkeypatch.setattr(_inputproj, "backward", lambda *a: calls.append(a))
    leaves = [x.detach().requires_grad_(True) for x in d["xs"]]
    tokens = op()(leaves, G, d["weights"], d["biases"])
    other = torch.ones(1, device=DEV, requires_grad=True)
    torch.autograd.grad((tokens * other).sum(), other)                 # nothing of the operator is asked for: no launch
    assert calls == []


def test_runs_under_deterministic_algorithms():
    import warnings
    N, C, G, levels = TAILS
    d = on_gpu(K.case(N, C, G, levels, 4.0)[0])
    want = K.run(d, op())
    torch.use_deterministic_algorithms(True)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = K.run(d, op())
    finally:
        torch.use_deterministic_algorithms(False)
    assert all_same_bits(got, want)


@pytest.mark.parametrize("mix", [(F32, F32, F32), (BF16, F32, F32)], ids=["float32", "autocast"])
def test_results_over_stale_memory_are_complete_and_stay_inside(monkeypatch, mix):
    """Tokens, statistics, gradients and the workspaces are handed out holding NaN payloads between guard zones: every element is
    written before it is read, and nothing outside is touched."""
    from devis_amd.functions import input_projection
    for N, C, G, levels in (FOUR, TAILS, (1, 260, 4, ((19, 27), (1, 1)))):
        d = on_gpu(K.case(N, C, G, levels, 0.0, mix)[0])
        clean = K.run(d, op(), out_dtype=mix[2])
        with monkeypatch.context() as m:
            shim = stale_memory.install(m, [input_projection])
            got = K.run(d, op(), out_dtype=mix[2])
            assert len(shim.buffers) >= 4 + 3 * len(levels) and shim.guards_intact()
        tensors = [got["tokens"]] + [t for name in GRADS for t in got[name]]
        assert all(bool(t.isfinite().all()) for t in tensors) and all_same_bits(got, clean)


def test_above_the_limits_the_composite_runs_and_agrees(monkeypatch):
    from devis_amd import _inputproj
    from devis_amd.functions import input_projection
    monkeypatch.setattr(_inputproj, "forward", lambda *a: pytest.fail("the kernel ran"))
    for N, C, G, levels in ((1, 1032, 8, ((2, 3),)), (1, 8, 2, ((2, 2),) * 9)):
        d, want = K.case(N, C, G, levels)
        assert not input_projection.takes_kernels(on_gpu(d)["xs"], G, on_gpu(d)["weights"])
        got = K.run(on_gpu(d), op())
        assert_close(got["tokens"], want["tokens"], 1e-4, "composite tokens")
        for name in GRADS:
            for g, w in zip(got[name], want[name]):
                assert_close(g, w, 1e-4, "composite " + name)


# ---- the patched model -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("autocast", [False, True], ids=["float32", "bfloat16-autocast"])
def test_patched_model_reproduces_the_fixture_on_the_gpu(monkeypatch, autocast):
    import devis_amd
    from devis_amd import _inputproj
    fixture = K.load_fixture()
    calls = []
    for name in ("forward", "backward"):
        monkeypatch.setattr(_inputproj, name, lambda *a, _f=getattr(_inputproj, name), _n=name: (calls.append(_n), _f(*a))[1])
    model, features = K.build_model(fixture, torch.float32, DEV)
    # the documented order: patch_transformer first, patch_position_encoding second; patch_input_proj is independent of both
    previous_points = devis_amd.patch_transformer(K)
    previous_position = devis_amd.patch_position_encoding(K, K)
    previous = devis_amd.patch_input_proj(model)
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            got, srcs, src_flatten = K.run_model(model, features, fixture)
    finally:
        devis_amd.unpatch_input_proj(model, previous)
        devis_amd.unpatch_position_encoding(K, K, previous_position)
        devis_amd.argument_builders.unpatch_transformer(K, previous_points)
    assert calls == ["forward", "backward"]                                     # ONE fused call each way for the four levels
    assert src_flatten.dtype == torch.float32 and src_flatten.is_contiguous()
    start = 0
    for src in srcs:                                                            # the bound views: no second copy
        assert isinstance(src, devis_amd.DeferredInputProjection)
        view = src.materialize()
        assert view.data_ptr() == src_flatten.data_ptr() + start * src_flatten.shape[2] * src_flatten.element_size()
        assert tuple(view.shape) == tuple(src.shape) and torch.equal(view.flatten(2).transpose(1, 2), src_flatten[:, start:start + view.shape[2] * view.shape[3]])
        start += view.shape[2] * view.shape[3]
    tol = 1e-2 if autocast else 1e-4
    for name, want in K.expected(fixture).items():
        if autocast and name == "src_flatten":
            # The fourth level's groups are 2 elements of a bfloat16 convolution output: rounding that output moves their
            # normalised values by up to 0.2 of max|want| in stock torch too (measured on the CPU), so under autocast that one
            # token is compared with the stock modules run on the same inputs instead, at the float32 bar.
            assert_close(got[name][:, :-1], want[:, :-1], tol, "model src_flatten but the last token")
            stock_model, stock_features = K.build_model(fixture, torch.float32, DEV)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                stock = K.run_model(stock_model, stock_features, fixture)[0]
            assert_close(got[name], stock[name].double().cpu(), 1e-4, "model src_flatten against the stock modules")
            continue
        assert_close(got[name], want, tol, "model " + name)
