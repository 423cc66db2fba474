"""GPU tests of the transformer layers' glue operators (include/addnorm.h) against the float64 oracle of
tests/addnorm_oracle.py, run on exactly the operands the operators received (16-bit inputs are rounded once, before both sides
see them).

Tolerance: max|got - want| <= tol * max|want| per tensor (tests/test_attmap_gpu.py::assert_close), tol = 1e-4 for a float32
result, 1e-2 for a bfloat16 / float16 one, 1e-10 for float64 -- the project's own bars, by the dtype a result is stored in.
Everything the mask rule, the fixed summation order and the recomputation promise is compared bit for bit."""
import warnings

import pytest
import torch

import addnorm_oracle as O
import layerglue_cases as L
import stale_memory
from test_attmap_gpu import TOL, assert_close
from test_unaligned_gpu import SHIFTS, canaries_intact, shifted

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
# (x, delta, out_dtype, parameters): every combination the kernels are instantiated for
COMBOS = [(F32, F32, None, F32), (F64, F64, None, F64), (BF16, BF16, None, BF16), (F16, F16, None, F16),
          (BF16, BF16, None, F32), (F16, F16, None, F32), (F32, BF16, None, F32), (F32, F16, None, F32),
          (BF16, BF16, F32, BF16), (F16, F16, F32, F16), (BF16, BF16, F32, F32), (F16, F16, F32, F32)]
CHANNELS = (256, 252, 32, 7, 1, 1024)
PROBABILITIES = (0.0, 0.1, 0.5, 1.0)
SEEDS = (0, 1, 20260101, 0x123456789ABCDEF, 2 ** 63 - 1)


def name_of(combo):
    return "-".join(str(d).replace("torch.", "") for d in combo)


def chunk_rows():
    from devis_amd import _addnorm
    return _addnorm.tile(_addnorm.TILE_ROWS)


def rows():
    return (1, 5, chunk_rows() + 1)


def seed_tensor(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def make_inputs(R, C, combo, seed=0):
    """(x, delta, weight, bias, grad_y) on the CPU in the combination's dtypes."""
    xd, dd, od, pd = combo
    g = torch.Generator().manual_seed(1000 * R + C + seed)
    shape = (R, C)
    x, delta = torch.randn(shape, generator=g, dtype=F64).to(xd), (0.5 * torch.randn(shape, generator=g, dtype=F64)).to(dd)
    weight, bias = (1 + 0.5 * torch.randn(C, generator=g, dtype=F64)).to(pd), torch.randn(C, generator=g, dtype=F64).to(pd)
    return x, delta, weight, bias, torch.randn(shape, generator=g, dtype=F64).to(od or xd)


def run_norm(x, delta, weight, bias, grad_y=None, p=0.0, seed=None, out_dtype=None, wants=(True,) * 4, eps=1e-5):
    """(y, grad_x, grad_delta, grad_weight, grad_bias) on the device; gradients not in ``wants`` are None."""
    import devis_amd
    ts = [t.to(DEV).requires_grad_(grad_y is not None and want) for t, want in zip((x, delta, weight, bias), wants)]
    y = devis_amd.add_layer_norm(*ts, eps, p=p, seed=None if seed is None else seed_tensor(seed), out_dtype=out_dtype)
    if grad_y is None:
        return (y,) + (None,) * 4
    asked = [t for t, want in zip(ts, wants) if want]
    grads = iter(torch.autograd.grad(y, asked, grad_y.to(DEV)))
    return (y.detach(),) + tuple(next(grads) if want else None for want in wants)


def same_bits(a, b):
    """Bit for bit, NaNs included."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def close(got, want, what):
    assert_close(got, want, TOL[got.dtype], what)


# ---- oracle parity ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", COMBOS, ids=name_of)
def test_add_layer_norm_matches_the_oracle(combo):
    xd, dd, od, pd = combo
    for R in rows():
        for C in CHANNELS:
            x, delta, weight, bias, grad_y = make_inputs(R, C, combo)
            for p in PROBABILITIES:
                seed = None if p == 0 else 20260101 + C
                keep = None if p == 0 else O.keep_mask(seed, R, C, p)
                got = run_norm(x, delta, weight, bias, grad_y, p, seed, od)
                want = O.add_layer_norm_grads(x, delta, weight, bias, 1e-5, grad_y, keep, O.scale_of(p) if p else 1.0)
                assert [t.dtype for t in got] == [od or xd, xd, dd, pd, pd]
                for name, g, w in zip(("y", "grad_x", "grad_delta", "grad_weight", "grad_bias"), got, want):
                    close(g, w, "%s R=%d C=%d p=%s %s" % (name_of(combo), R, C, p, name))


@pytest.mark.parametrize("dtype", [F32, F64, BF16, F16], ids=str)
def test_relu_dropout_matches_the_oracle(dtype):
    import devis_amd
    for R in rows():
        for C in CHANNELS + (1030,):
            g = torch.Generator().manual_seed(R + C)
            x, grad_y = torch.randn(R, C, generator=g, dtype=F64).to(dtype), torch.randn(R, C, generator=g, dtype=F64).to(dtype)
            for p in PROBABILITIES:
                seed = None if p == 0 else 77 + C
                keep = None if p == 0 else O.keep_mask(seed, R, C, p)
                xg = x.to(DEV).requires_grad_(True)
                y = devis_amd.relu_dropout(xg, p=p, seed=None if p == 0 else seed_tensor(seed))
                gx, = torch.autograd.grad(y, xg, grad_y.to(DEV))
                assert y.dtype == dtype and gx.dtype == dtype
                close(y.detach(), O.relu_dropout(x, keep, O.scale_of(p)), "%s R=%d C=%d p=%s y" % (dtype, R, C, p))
                close(gx, O.relu_dropout_grad(x, grad_y, keep, O.scale_of(p)), "%s R=%d C=%d p=%s grad_x" % (dtype, R, C, p))
                if keep is not None:
                    assert not y.detach().cpu()[~keep].any()                              # a dropped element is exactly 0


@pytest.mark.parametrize("kind", ["encoder", "decoder"])
def test_patched_stand_in_layers_reproduce_the_reference_fixtures(kind):
    import devis_amd
    case, module = L.load_case(kind), L.reference_module()
    undo = devis_amd.patch_transformer_layers(module)
    try:
        got = L.run_case(module, kind, case, DEV, F32)
    finally:
        devis_amd.unpatch_transformer_layers(module, undo)
    for key, value in got.items():
        close(value, case[key], "%s %s" % (kind, key))


# ---- the mask ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, F64], ids=str)
def test_the_mask_is_the_oracles_bit_for_bit(dtype):
    import devis_amd
    combo = (dtype, dtype, None, dtype)
    for seed in SEEDS + (-1, -(2 ** 63)):
        for R, C, p in ((5, 256, 0.1), (chunk_rows() + 1, 252, 0.5), (5, 7, 0.5), (1, 1024, 0.1), (5, 1, 0.5), (5, 32, 1.0)):
            x, delta, weight, bias, grad_y = make_inputs(R, C, combo)
            keep, scale = O.keep_mask(seed, R, C, p), O.scale_of(p)
            got = run_norm(x, delta, weight, bias, grad_y, p, seed)
            masked = torch.where(keep, delta * scale, torch.zeros_like(delta))
            want = run_norm(x, masked, weight, bias, grad_y, 0.0, None)
            what = "seed %d R=%d C=%d p=%s" % (seed, R, C, p)
            for i in (0, 1, 3, 4):                                       # y and every gradient but grad_delta
                assert same_bits(got[i], want[i]), (what, i)
            grad_delta = torch.where(keep.to(DEV), want[2] * scale, torch.zeros_like(want[2]))
            assert same_bits(got[2], grad_delta), what
            ones = torch.ones(R, C, dtype=dtype, device=DEV)
            y = devis_amd.relu_dropout(ones, p=p, seed=seed_tensor(seed))
            assert same_bits(y, torch.where(keep.to(DEV), torch.full_like(ones, scale), torch.zeros_like(ones))), what


def test_the_kept_count_is_within_four_sigma_and_the_device_equals_the_oracle():
    """A condition on the generator, asserted on the oracle; the device only has to equal the oracle."""
    import devis_amd
    for seed in SEEDS:
        for R, C, p in ((65, 256, 0.1), (65, 256, 0.5), (33, 252, 0.1), (130, 1024, 0.1), (9, 7, 0.5)):
            keep = O.keep_mask(seed, R, C, p)
            n, kept = R * C, int(keep.sum())
            sigma = (n * p * (1 - p)) ** 0.5
            print("seed %d R=%d C=%d p=%s: kept %d of %d, %.2f sigma" % (seed, R, C, p, kept, n, abs(kept - n * (1 - p)) / sigma))
            assert abs(kept - n * (1 - p)) <= 4 * sigma
            y = devis_amd.relu_dropout(torch.ones(R, C, device=DEV), p=p, seed=seed_tensor(seed))
            assert torch.equal(y.cpu() != 0, keep)


# ---- reproducibility --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", [COMBOS[0], COMBOS[2], COMBOS[6]], ids=name_of)
def test_results_are_bitwise_reproducible_and_rows_and_gradients_are_independent(combo):
    R, C = 3 * chunk_rows() + 1, 252
    x, delta, weight, bias, grad_y = make_inputs(R, C, combo)
    for p in (0.0, 0.5, 1.0):
        seed = None if p == 0 else 11
        full = run_norm(x, delta, weight, bias, grad_y, p, seed, combo[2])
        again = run_norm(x, delta, weight, bias, grad_y, p, seed, combo[2])
        assert all(same_bits(a, b) for a, b in zip(full, again)), p
        for i in range(4):                                               # each gradient alone
            wants = tuple(j == i for j in range(4))
            alone = run_norm(x, delta, weight, bias, grad_y, p, seed, combo[2], wants)
            assert same_bits(alone[0], full[0]) and same_bits(alone[1 + i], full[1 + i]), (p, i)
            assert all(alone[1 + j] is None for j in range(4) if j != i)
        pair = run_norm(x, delta, weight, bias, grad_y, p, seed, combo[2], (False, False, True, True))
        assert same_bits(pair[3], full[3]) and same_bits(pair[4], full[4])
    full = run_norm(x, delta, weight, bias, grad_y, 0.0, None, combo[2])
    for r in (0, chunk_rows(), R - 1):                                   # a row alone and in the batch
        one = run_norm(x[r:r + 1], delta[r:r + 1], weight, bias, grad_y[r:r + 1], 0.0, None, combo[2])
        assert same_bits(one[0], full[0][r:r + 1]) and same_bits(one[1], full[1][r:r + 1]), r
    # leading dimensions only flatten
    lead = run_norm(x.view(1, R, C), delta.view(1, R, C), weight, bias, grad_y.view(1, R, C), 0.5, 11, combo[2])
    flat = run_norm(x, delta, weight, bias, grad_y, 0.5, 11, combo[2])
    assert all(same_bits(a.view(b.shape), b) for a, b in zip(lead, flat))


def test_relu_dropout_is_bitwise_reproducible():
    import devis_amd
    x = torch.randn(67, 1030, device=DEV)
    a, b = (devis_amd.relu_dropout(x, p=0.3, seed=seed_tensor(5)) for _ in range(2))
    assert same_bits(a, b) and not same_bits(a, devis_amd.relu_dropout(x, p=0.3, seed=seed_tensor(6)))


# ---- special values ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, F64, BF16, F16], ids=str)
def test_a_constant_row_gives_the_bias_exactly_and_finite_gradients(dtype):
    for C in (256, 252, 7, 1, 1024):
        x, delta, weight, bias, grad_y = make_inputs(5, C, (dtype, dtype, None, dtype))
        x[2], delta[2] = 0.25, 0.75                                      # x + delta == 1.0 everywhere
        y, gx, gd, gw, gb = run_norm(x, delta, weight, bias, grad_y)
        assert same_bits(y[2].cpu(), bias), C
        assert all(bool(t.isfinite().all()) for t in (y, gx, gd, gw, gb)), C


def test_a_nan_or_inf_changes_its_own_row_only():
    import devis_amd
    R, C = chunk_rows() + 3, 252
    x, delta, weight, bias, grad_y = make_inputs(R, C, COMBOS[0])
    clean = run_norm(x, delta, weight, bias, grad_y, 0.5, 3)
    for value, where in ((float("nan"), "x"), (float("inf"), "x"), (float("-inf"), "delta")):
        bad_x, bad_delta = x.clone(), delta.clone()
        cols = [c for c in range(C) if O.keep_mask(3, R, C, 0.5)[4, c]][:2]           # kept elements: a dropped one is exactly 0
        (bad_x if where == "x" else bad_delta)[4, cols[0]] = value
        got = run_norm(bad_x, bad_delta, weight, bias, grad_y, 0.5, 3)
        others = [r for r in range(R) if r != 4]
        for i in (0, 1):                                                 # y and grad_x
            assert same_bits(got[i][others], clean[i][others]), (value, i)
            assert not bool(got[i][4].isfinite().all()), (value, i)
    # a dropped NaN or Inf in delta changes nothing at all
    dropped = [c for c in range(C) if not O.keep_mask(3, R, C, 0.5)[4, c]][0]
    bad_delta = delta.clone()
    bad_delta[4, dropped] = float("nan")
    assert all(same_bits(a, b) for a, b in zip(run_norm(x, bad_delta, weight, bias, grad_y, 0.5, 3), clean))
    # relu_dropout: a kept NaN stays NaN, a dropped one is exactly 0, and the gradient there is 0
    keep = O.keep_mask(9, 4, 40, 0.5)
    h = torch.full((4, 40), float("nan"), device=DEV, requires_grad=True)
    y = devis_amd.relu_dropout(h, p=0.5, seed=seed_tensor(9))
    assert torch.equal(y.detach().isnan().cpu(), keep) and not y.detach().cpu()[~keep].any()
    assert not torch.autograd.grad(y, h, torch.ones_like(y))[0].any()
    inf = torch.full((4, 40), float("inf"), device=DEV)
    assert torch.equal(devis_amd.relu_dropout(inf, p=0.5, seed=seed_tensor(9)).cpu(), torch.where(keep, float("inf"), 0.0))
    assert not devis_amd.relu_dropout(-inf).any()


# ---- placement --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", [COMBOS[0], COMBOS[1], COMBOS[2], COMBOS[7]], ids=name_of)
def test_unaligned_and_non_dense_views_give_the_aligned_calls_bits(combo):
    import devis_amd
    xd, dd, od, pd = combo
    R, C = chunk_rows() + 2, 256
    x, delta, weight, bias, grad_y = make_inputs(R, C, combo)
    seed = seed_tensor(21)
    dev = [t.to(DEV) for t in (x, delta, weight, bias, grad_y)]

    def run(ts):
        leaves = [t.detach().requires_grad_(True) for t in ts[:4]]
        y = devis_amd.add_layer_norm(*leaves, p=0.5, seed=seed, out_dtype=od)
        return (y.detach(),) + torch.autograd.grad(y, leaves, ts[4])

    want = run(dev)
    for which in range(5):                                               # one operand at a time off the 16-byte boundary
        for k in SHIFTS[dev[which].dtype][:2]:
            view, buf = shifted(dev[which], k)
            got = run([view if i == which else t for i, t in enumerate(dev)])
            assert all(same_bits(a, b) for a, b in zip(got, want)), (which, k)
            canaries_intact(buf, k, dev[which].numel())
    # non-dense views: every other row of a taller tensor, a transposed tensor, a strided parameter
    tall = torch.zeros(2 * R, C, dtype=xd, device=DEV)
    tall[::2] = dev[0]
    wide = dev[1].t().contiguous().t()
    every_other = torch.zeros(2 * C, dtype=pd, device=DEV)
    every_other[::2] = dev[2]
    assert not tall[::2].is_contiguous() and not wide.is_contiguous() and not every_other[::2].is_contiguous()
    got = run([tall[::2], wide, every_other[::2], dev[3], dev[4].t().contiguous().t()])
    assert all(same_bits(a, b) for a, b in zip(got, want))
    # the relu pass
    h = dev[0]
    want = devis_amd.relu_dropout(h, p=0.5, seed=seed)
    for k in SHIFTS[xd][:2]:
        view, buf = shifted(h, k)
        assert same_bits(devis_amd.relu_dropout(view, p=0.5, seed=seed), want)
        canaries_intact(buf, k, h.numel())
    assert same_bits(devis_amd.relu_dropout(tall[::2], p=0.5, seed=seed), want)


@pytest.mark.parametrize("combo", [COMBOS[0], COMBOS[1], COMBOS[2], COMBOS[6], COMBOS[9]], ids=name_of)
def test_stale_outputs_and_workspace_are_fully_written_and_nothing_outside(monkeypatch, combo):
    import devis_amd
    from devis_amd.functions import add_norm
    xd, dd, od, pd = combo
    cases = [(3 * chunk_rows() + 1, 252, 0.5), (chunk_rows(), 7, 0.1), (5, 1024, 0.0), (chunk_rows() + 1, 1, 1.0)]
    clean = [run_norm(*make_inputs(R, C, combo), p=p, seed=None if p == 0 else 4, out_dtype=od) for R, C, p in cases]
    h = torch.randn(37, 1030, dtype=F64).to(xd).to(DEV)
    clean_relu = devis_amd.relu_dropout(h, p=0.5, seed=seed_tensor(4))
    shim = stale_memory.install(monkeypatch, [add_norm])
    for (R, C, p), want in zip(cases, clean):
        x, delta, weight, bias, grad_y = make_inputs(R, C, combo)
        got = run_norm(x, delta, weight, bias, grad_y, p, None if p == 0 else 4, od)
        assert all(same_bits(a, b) for a, b in zip(got, want)), (R, C, p)
        for wants in ((True, False, False, False), (False, False, True, False)):
            got = run_norm(x, delta, weight, bias, grad_y, p, None if p == 0 else 4, od, wants)
            assert all(g is None or same_bits(g, w) for g, w in zip(got, want)), (R, C, p, wants)
    hg = h.clone().requires_grad_(True)
    y = devis_amd.relu_dropout(hg, p=0.5, seed=seed_tensor(4))
    gx, = torch.autograd.grad(y, hg, torch.ones_like(y))
    assert same_bits(y.detach(), clean_relu) and bool(gx.isfinite().all())
    assert len(shim.buffers) > 20 and shim.guards_intact()


# ---- graphs, synchronisation, determinism -----------------------------------------------------------------------------------------

def test_a_captured_training_call_replayed_after_seed_copy_equals_the_eager_call_with_the_new_seed():
    import devis_amd
    R, C = chunk_rows() + 1, 256
    x, delta, weight, bias, grad_y = (t.to(DEV) for t in make_inputs(R, C, COMBOS[0]))
    seed = seed_tensor(100)

    def step():
        leaves = [t.detach().requires_grad_(True) for t in (x, delta, weight, bias)]
        y = devis_amd.add_layer_norm(*leaves, p=0.1, seed=seed)
        h = devis_amd.relu_dropout(y, p=0.1, seed=seed)
        return (y.detach(), h.detach()) + torch.autograd.grad(h, leaves, grad_y)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    results = {}
    for value in (100, 20260101, -5):
        seed.copy_(seed_tensor(value))
        graph.replay()
        torch.cuda.synchronize()
        results[value] = [t.clone() for t in captured]
        eager = step()
        assert all(same_bits(a, b) for a, b in zip(results[value], eager)), value
    assert not same_bits(results[100][0], results[20260101][0]) and not same_bits(results[100][1], results[-5][1])


def attention_stub(shape):
    value = torch.nn.Parameter(torch.randn(shape, device=DEV))
    return lambda *args, **kwargs: (value, None)


def test_patched_layers_train_without_host_synchronisation_and_under_the_determinism_flag():
    import devis_amd
    module = L.reference_module()
    torch.manual_seed(3)
    encoder = module.DeformableTransformerEncoderLayer().to(DEV).train()
    decoder = module.DeformableTransformerDecoderLayer().to(DEV).train()
    encoder.self_attn = attention_stub((2, 7, L.D_MODEL))
    decoder.cross_attn = attention_stub((1, 6, L.D_MODEL))
    src, pos = torch.randn(2, 7, L.D_MODEL, device=DEV, requires_grad=True), torch.randn(2, 7, L.D_MODEL, device=DEV)
    tgt, query_pos = torch.randn(1, 6, L.D_MODEL, device=DEV, requires_grad=True), torch.randn(1, 6, L.D_MODEL, device=DEV)

    def step():
        out = encoder(src, pos, None, None, None).sum() + decoder(tgt, query_pos, None, None, None, None).sum()
        out.backward()
        return out

    undo = devis_amd.patch_transformer_layers(module)
    try:
        step()                                                           # (loads the library, warms the allocator)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            outs = [step() for _ in range(3)]
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert all(bool(o.isfinite()) for o in outs) and bool(src.grad.isfinite().all()) and encoder.norm1.weight.grad is not None
        assert float(outs[0].detach()) != float(outs[1].detach())                          # a new mask every call
        torch.use_deterministic_algorithms(True)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                step()
                x, delta, weight, bias, grad_y = make_inputs(chunk_rows() + 1, 252, COMBOS[0])
                run_norm(x, delta, weight, bias, grad_y, 0.5, 1)
                h = torch.randn(5, 64, device=DEV, requires_grad=True)
                devis_amd.relu_dropout(h, p=0.5, seed=seed_tensor(1)).sum().backward()
        finally:
            torch.use_deterministic_algorithms(False)
        encoder.eval()
        a, b = encoder(src, pos, None, None, None), encoder(src, pos, None, None, None)
        assert same_bits(a.detach(), b.detach())
    finally:
        devis_amd.unpatch_transformer_layers(module, undo)


def test_more_than_1024_channels_raise_before_any_launch():
    import devis_amd
    x = torch.zeros(2, 1025, device=DEV)
    with pytest.raises(RuntimeError, match="1 to 1024 channels"):
        devis_amd.add_layer_norm(x, x, torch.ones(1025, device=DEV), torch.zeros(1025, device=DEV))
    with pytest.raises(ValueError, match="needs a seed"):
        devis_amd.relu_dropout(x, p=0.5)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.relu_dropout(x, p=0.5, seed=torch.zeros(1, dtype=torch.int64))
    assert devis_amd.add_layer_norm(x[:0, :8], x[:0, :8], torch.ones(8, device=DEV), torch.zeros(8, device=DEV)).shape == (0, 8)
