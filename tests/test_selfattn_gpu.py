"""GPU tests of the decoder's query self-attention kernels (include/selfattn.h) against the float64 oracle of
tests/selfattn_oracle.py, fed the same (already rounded) inputs.

Tolerance: max|got - want| <= tol * max|want| per tensor (tests/test_attmap_gpu.py::assert_close), tol = 1e-4 for a float32
result and 1e-2 for a bfloat16 / float16 one -- the project's own bars, by the dtype a result is stored in.  Plain float32 torch
deviates from float64 by at most 4.2e-6 of max|want| at these shapes (output and all three gradients), so the float32 bar
leaves a twenty-fold margin.  Everything the mask rule, the fixed summation order, the views and the recomputation promise is
compared bit for bit."""
import warnings

import pytest
import torch
from torch import nn

import layerglue_cases as LG
import selfattn_cases as C
import selfattn_oracle as O
import stale_memory
from test_attmap_gpu import TOL, assert_close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
SIZES = [(1, 1), (16, 16), (17, 15), (33, 70), (300, 300)]                 # (L, S): every tile edge, and the reference's
HEADS = [(1, 8, 32), (3, 1, 4), (2, 8, 4), (2, 3, 20), (1, 2, 64)]          # (N, H, D): CT = 2, 1, 1, 2, 4 (CT = 3 and every other
#                                                                            D: the matrices below), the reference's first


make_inputs, run = C.make_inputs, C.run


def seed_tensor(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def compare(got, want, operands, D, dtype, p=0.0, what="", cancelling=()):
    """``got`` against the oracle's ``want`` at the bars.  Beside an all-zero oracle, and for the tensors named in
    ``cancelling``, the bar is tol times the size of the terms that cancel."""
    q, k, v, go = operands
    for name, a, b in zip(C.NAMES, got, want):
        assert a.dtype == dtype and a.shape == b.shape and a.is_contiguous()
        if name in cancelling or float(b.abs().max()) == 0.0:
            # S == 1 (grad_q and grad_k are dS = P (dP - delta) times k or q, and dP == delta in exact arithmetic), one-hot rows
            # (the same, up to what underflows) or p == 1 (everything is dropped): tests/selfattn_cases.py::cancelling_terms
            terms = C.cancelling_terms(q, k, v, go, D, p)
            err = float((a.double().cpu() - b).abs().max())
            print("%s %s: max error %.3e beside an oracle of max %.3e, cancelling terms %.3e" % (what, name, err, float(b.abs().max()), terms))
            assert bool(a.isfinite().all()) and err <= TOL[dtype] * terms, (what, name, err)
        else:
            assert_close(a, b, TOL[dtype], "%s %s" % (what, name))


def check(L, S, N, H, D, dtype=F32, gain=1.0, p=0.0, seed=None, what=""):
    q, k, v, go = make_inputs(L, S, N, H, D, dtype, gain)
    keep = None if not p else O.keep_mask(seed, N, H, L, S, p)
    want = O.attention_grads(q, k, v, H, go, keep, O.scale_of(p))
    got = run(*(t.to(DEV) for t in (q, k, v, go)), H, p, None if not p else seed_tensor(seed))
    compare(got, want, (q, k, v, go), D, dtype, p, what)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ---- oracle parity -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,H,D", HEADS)
@pytest.mark.parametrize("L,S", SIZES)
def test_float32_matches_the_oracle(L, S, N, H, D):
    check(L, S, N, H, D, what="L %d S %d N %d H %d D %d" % (L, S, N, H, D))


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("L,S,N,H,D", [(33, 70, 2, 8, 32), (17, 15, 3, 1, 4)])
def test_16_bit_operands_match_the_oracle(L, S, N, H, D, dtype):
    check(L, S, N, H, D, dtype, what=str(dtype))


def test_large_logits_stay_within_the_bound():
    check(70, 70, 1, 2, 32, gain=30.0, what="queries x 30")


# ---- every compiled variant (tests/selfattn_cases.py lists them; tests/test_selfattn_cpu.py asserts that these lists launch all
# 36 and that a correct implementation stays within half of each bar on them) ----------------------------------------------------

def check_operands(operands, H, D, dtype, p=0.0, seed=None, what="", cancelling=()):
    """The operator on ``operands`` (GPU tensors, passed as the views they are) against the oracle on their values."""
    dense = [t.contiguous().cpu() for t in operands]
    L, N, S = dense[0].shape[0], dense[0].shape[1], dense[1].shape[0]
    keep = None if not p else O.keep_mask(seed, N, H, L, S, p)
    want = O.attention_grads(*dense[:3], H, dense[3], keep, O.scale_of(p))
    got = run(*operands, H, p, None if not p else seed_tensor(seed))
    compare(got, want, dense, D, dtype, p, what, cancelling)


@pytest.mark.parametrize("L,S,N,H,D", C.MATRIX_F32)
def test_every_head_dimension_matches_the_oracle_in_float32(L, S, N, H, D):
    """N, H = 2, 3: the head offset h * D is no multiple of 16 for most D."""
    check(L, S, N, H, D, what="L %d S %d D %d" % (L, S, D))


@pytest.mark.parametrize("L,S,N,H,D,dtype,p", C.MATRIX_16)
def test_every_tile_count_matches_the_oracle_in_16_bit_with_and_without_dropout(L, S, N, H, D, dtype, p):
    check(L, S, N, H, D, dtype, p=p, seed=C.DROPOUT_SEED, what="%s D %d p %s" % (dtype, D, p))


@pytest.mark.parametrize("S,dtype,p,last,boost", C.PLANTED)
def test_planted_row_maxima_in_the_first_and_in_the_last_partly_masked_tile(S, dtype, p, last, boost):
    """Key 0 or S - 1 (the last tile holds 1 key of 16) gains ``boost`` on every logit.  At 9 the softmax is peaked and every
    tensor meets its bar.  At 60 every later (or earlier) exp underflows against it and rows are one-hot: grad_q and grad_k are
    pure cancellation -- of the order 1e-23 in the float64 oracle, and float32 torch is off by 100 % of that -- so they are
    held to the bound on cancelling terms and out and grad_v to their bars.  While the backward took delta from the rounded
    out, boost 9 left grad_q off by 1.5 % to 3.5 % of max|want| in every bfloat16 case and grad_k by 1.0 % in one float16 case
    ("What is saved")."""
    L, N, H, D = C.PLANTED_SHAPE
    operands = C.planted_inputs(L, S, N, H, D, dtype, S - 1 if last else 0, boost)
    check_operands([t.to(DEV) for t in operands], H, D, dtype, p, C.DROPOUT_SEED, "S %d %s p %s key %s boost %d" % (
        S, dtype, p, "S - 1" if last else "0", boost), cancelling=("grad_q", "grad_k") if boost > 9 else ())


@pytest.mark.parametrize("L,S,N,H,D,p", C.LOPSIDED)
def test_lopsided_sizes_match_the_oracle(L, S, N, H, D, p):
    check(L, S, N, H, D, p=p, seed=C.DROPOUT_SEED, what="L %d S %d p %s" % (L, S, p))


@pytest.mark.parametrize("seed", C.SWEEP)
def test_sweep_through_views_matches_the_oracle(seed):
    c = C.sweep_config(seed)
    dense = [t.to(DEV) for t in make_inputs(c.L, c.S, c.N, c.H, c.D, c.dtype, seed=seed)]
    check_operands(C.VIEWS[c.view].build(*dense), c.H, c.D, c.dtype, c.p, c.dropout_seed, str(c))


# ---- views -------------------------------------------------------------------------------------------------------------------

def test_views_give_the_bits_of_dense_aligned_copies():
    L, S, N, H, D = 33, 33, 2, 8, 32
    E = H * D
    q, k, v, go = (t.to(DEV) for t in make_inputs(L, S, N, H, D))
    want = run(q, k, v, go, H)
    # q and k as the halves of one packed [L, N, 2E] tensor
    packed = torch.cat([q, k], -1)
    pq, pk = packed[..., :E], packed[..., E:]
    assert pq.stride() == (2 * N * E, 2 * E, 1) and pk.data_ptr() != pq.data_ptr()
    # batch_first tensors, transposed
    bq, bk, bv = (t.transpose(0, 1).contiguous().transpose(0, 1) for t in (q, k, v))
    assert bq.stride() == (E, L * E, 1)
    # operands one element into their storage: not 16-byte aligned
    def shifted(t):
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        flat[1:].copy_(t.reshape(-1))
        return flat[1:].view(t.shape)
    sq, sk, sv, sgo = (shifted(t) for t in (q, k, v, go))
    assert sq.data_ptr() % 16 == 4
    # rows 12 channels apart more: strides that are no multiple of 4 are fine too (3 elements of padding per row)
    wide = torch.zeros(S, N, E + 3, device=DEV)
    wide[..., :E] = v
    for name, args in (("packed", (pq, pk, v, go)), ("batch_first", (bq, bk, bv, go)), ("shifted", (sq, sk, sv, sgo)),
                       ("padded rows", (q, k, wide[..., :E], go))):
        got = run(*args, H)
        for what, a, b in zip(("out", "grad_q", "grad_k", "grad_v"), got, want):
            assert same_bits(a, b), (name, what)
    # 16-bit: 8-byte accesses against per-element ones
    hq, hk, hv, hgo = (t.to(BF16) for t in (q, k, v, go))
    want = run(hq, hk, hv, hgo, H)
    got = run(shifted(hq), shifted(hk), shifted(hv), shifted(hgo), H)
    assert all(same_bits(a, b) for a, b in zip(got, want)) and shifted(hq).data_ptr() % 16 == 2


@pytest.mark.parametrize("D,dtype", C.VIEW_MATRIX)
def test_every_view_gives_the_bits_of_the_dense_call_at_every_variant(D, dtype):
    """What the test above promises at D = 32, for every CT, with and without the vector chunk path, in every storage type and
    with dropout: the per-element path ("shifted", "padded_rows", "only_v_unaligned", and "packed" where the k half is not
    16-byte aligned) and the 8 / 16-byte one give the same bits.  "broadcast" -- batch strides of 0 -- changes the values and
    is compared with the call on dense copies of its operands."""
    L, S, N, H = C.VIEW_SHAPE
    dense = C.VIEWS["dense"].build(*(t.to(DEV) for t in make_inputs(L, S, N, H, D, dtype)))
    assert C.aligned_and_quad_strided(*dense)
    seed = seed_tensor(C.DROPOUT_SEED)
    want = run(*dense, H, 0.5, seed)
    for name, view in C.VIEWS.items():
        operands = view.build(*dense)
        assert C.aligned_and_quad_strided(*operands) is view.vec(H * D, dtype), name
        ref = want if name != "broadcast" else run(*(t.contiguous() for t in operands), H, 0.5, seed)
        got = run(*operands, H, 0.5, seed)
        for what, a, b in zip(C.NAMES, got, ref):
            assert same_bits(a, b), (name, what)
    assert not all(same_bits(a, b) for a, b in zip(ref, want))                    # (the broadcast operands are other values)


def test_guard_zones_stay_untouched_and_results_are_fully_written(monkeypatch):
    from devis_amd import _native, _selfattn
    L, S, N, H, D, G = 33, 21, 2, 3, 20, 64
    E = H * D
    q, k, v, go = (t.to(DEV) for t in make_inputs(L, S, N, H, D))
    want = run(q, k, v, go, H, 0.5, seed_tensor(3))

    def guarded(shape, dtype=F32, fill=None):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 2 * G,), float("nan"), dtype=dtype, device=DEV)
        inner = buf[G:G + n].view(shape)
        if fill is not None:
            inner.copy_(fill)
        return buf, inner

    _, (gq, gk, gv, ggo) = zip(*(guarded(t.shape, fill=t) for t in (q, k, v, go)))
    outs = [guarded((L, N, E)), guarded((N * H, L)), guarded((L, N, E)), guarded((S, N, E)), guarded((S, N, E))]
    (_, out), (_, lse), (_, dq), (_, dk), (_, dv) = outs
    shape, seed = _selfattn.Shape(L, S, N, E, H), seed_tensor(3)
    assert _selfattn.forward(_native.dtype_code(F32), gq, gk, gv, seed, 0.5, shape, out, lse) == 1
    assert _selfattn.backward(_native.dtype_code(F32), gq, gk, gv, out, ggo, lse, seed, 0.5, shape, dq, dk, dv) == 2
    torch.cuda.synchronize()
    for name, a, b in zip(("out", "grad_q", "grad_k", "grad_v"), (out, dq, dk, dv), want):
        assert same_bits(a.contiguous(), b), name                                  # every element written, from the operands alone
    assert bool(lse.isfinite().all())
    for buf, inner in outs:
        assert bool(buf[:G].isnan().all()) and bool(buf[G + inner.numel():].isnan().all())
    # results allocated over stale memory (tests/stale_memory.py): NaN payloads between guard zones
    from devis_amd.functions import self_attention
    shim = stale_memory.install(monkeypatch, [self_attention])
    got = run(q, k, v, go, H, 0.5, seed_tensor(3))
    assert all(same_bits(a, b) for a, b in zip(got, want))
    assert len(shim.buffers) == 5 and shim.guards_intact()                      # out, lse and the three gradients


# ---- dropout -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [0.1, 0.5, 1.0])
def test_dropout_matches_the_oracle_with_the_restated_mask(p):
    check(33, 70, 2, 8, 32, p=p, seed=20260101, what="p %s" % p)
    check(17, 15, 3, 1, 4, p=p, seed=-7, what="p %s" % p)


@pytest.mark.parametrize("D", [64, 20, 48])
@pytest.mark.parametrize("p", [0.1, 0.5, 1.0])
def test_the_mask_is_read_back_exactly(p, D):
    """q = 0 gives uniform probabilities 1 / S, and with v_h the identity (S = D) out[i, n, h * D + j] is
    keep(n, h, i, j) * scale / S.  S = D = 64 is four full tiles, 20 ends in a Philox quad past a tile edge, 48 is CT = 3."""
    import devis_amd
    L, N, H = 37, 2, 2
    S, value = D, -0x123456789ABCDEF
    v = torch.eye(D, device=DEV)[:, None, None, :].expand(S, N, H, D).reshape(S, N, H * D).contiguous()
    out = devis_amd.multihead_attention(torch.zeros(L, N, H * D, device=DEV), torch.randn(S, N, H * D, device=DEV), v, H, p=p,
                                        seed=seed_tensor(value))
    got = out.view(L, N, H, D).permute(1, 2, 0, 3).cpu()
    keep = O.keep_mask(value, N, H, L, S, p)
    assert torch.equal(got != 0, keep)
    # the sum of a row's S ones is exact; the kernels multiply by its float32 reciprocal (exact for S = 64, not for 20 and 48)
    kept = torch.tensor(O.scale_of(p), dtype=F32) * (torch.ones((), dtype=F32) / S)
    assert torch.equal(got, torch.where(keep, kept, torch.zeros(())))


def test_the_seed_decides_the_mask_also_in_a_replayed_graph():
    L, S, N, H, D = 33, 33, 1, 8, 32
    q, k, v, go = (t.to(DEV) for t in make_inputs(L, S, N, H, D))
    seed = seed_tensor(100)
    step = lambda: run(q, k, v, go, H, 0.1, seed)      # noqa: E731
    first, again = step(), step()
    assert all(same_bits(a, b) for a, b in zip(first, again))
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
        assert all(same_bits(a, b) for a, b in zip(results[value], step())), value
    assert all(same_bits(a, b) for a, b in zip(results[100], first))
    for i in range(4):
        assert not same_bits(results[100][i], results[20260101][i]) and not same_bits(results[100][i], results[-5][i])


# ---- reproducibility -------------------------------------------------------------------------------------------------------------

def test_results_are_reproducible_and_independent_of_the_other_batch_entries():
    L, S, N, H, D = 33, 70, 3, 8, 32
    q, k, v, go = (t.to(DEV) for t in make_inputs(L, S, N, H, D))
    first = run(q, k, v, go, H, 0.5, seed_tensor(9))
    torch.use_deterministic_algorithms(True)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            again = run(q, k, v, go, H, 0.5, seed_tensor(9))
    finally:
        torch.use_deterministic_algorithms(False)
    assert all(same_bits(a, b) for a, b in zip(first, again))
    whole = run(q, k, v, go, H)
    for n in range(N):
        part = run(*(t[:, n:n + 1].contiguous() for t in (q, k, v, go)), H)
        for name, a, b in zip(("out", "grad_q", "grad_k", "grad_v"), whole, part):
            assert same_bits(a[:, n:n + 1].contiguous(), b), (n, name)


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_gradient_subsets_equal_the_full_run_and_launch_what_they_need(monkeypatch, p):
    from devis_amd import _selfattn
    L, S, N, H, D = 33, 70, 2, 3, 20
    q, k, v, go = (t.to(DEV) for t in make_inputs(L, S, N, H, D))
    seed = seed_tensor(5) if p else None
    launches = []
    real = _selfattn.backward
    monkeypatch.setattr(_selfattn, "backward", lambda *a: launches.append(real(*a)) or launches[-1])
    full = run(q, k, v, go, H, p, seed)
    assert launches == [2]
    for wants, count in (((True, False, False), 1), ((False, True, False), 1), ((False, False, True), 1), ((False, True, True), 1),
                         ((True, False, True), 2)):
        del launches[:]
        got = run(q, k, v, go, H, p, seed, wants)
        assert launches == [count], wants
        for a, b, want in zip(got[1:], full[1:], wants):
            assert (a is None) if not want else same_bits(a, b), wants
    del launches[:]
    run(q, k, v, go, H, p, seed, (False, False, False))
    assert launches == []


def test_nan_poisons_its_row_or_its_head_and_the_call_returns():
    L, S, N, H, D = 33, 33, 2, 4, 8
    q, k, v, go = (t.to(DEV) for t in make_inputs(L, S, N, H, D))
    q[5, 1, 2 * D + 3] = float("nan")                      # query 5 of (n 1, h 2)
    out = run(q, k, v, go, H)[0].view(L, N, H, D)
    bad = out.isnan()
    assert bool(bad[5, 1, 2].all()) and int(bad.sum()) == D
    q, k, v, go = (t.to(DEV) for t in make_inputs(L, S, N, H, D))
    k[21, 0, 1 * D + 7] = float("nan")                     # a key of (n 0, h 1)
    out = run(q, k, v, go, H)[0].view(L, N, H, D)
    bad = out.isnan()
    assert bool(bad[:, 0, 1].all()) and int(bad.sum()) == L * D
    torch.cuda.synchronize()


# ---- the module ------------------------------------------------------------------------------------------------------------------

def stock_and_fused(E, H, state=None, dropout=0.0, unit_biases=True, batch_first=False):
    """(float64 stock module on the CPU, fused module on the GPU) with equal parameters: ``state``, or torch's initialisation
    with, unless ``unit_biases`` is false, unit-normal biases in place of its zeros."""
    import devis_amd
    torch.manual_seed(2)
    stock = nn.MultiheadAttention(E, H, dropout=dropout, batch_first=batch_first).double().eval()
    if state is not None:
        stock.load_state_dict(state)
    elif unit_biases:
        with torch.no_grad():
            stock.in_proj_bias.normal_()
            stock.out_proj.bias.normal_()
    fused = devis_amd.FusedMultiheadAttention(E, H, dropout=dropout, batch_first=batch_first).eval()
    fused.load_state_dict(stock.state_dict())
    return stock, fused.to(DEV)


def module_results(module, x, value, grad_out, key=None):
    """The module on (x, x, value), or on (x, key, value) with a separate key, whose gradient is then "grad.key"."""
    leaves = [t.detach().requires_grad_(True) for t in ((x, value) if key is None else (x, value, key))]
    out, weights = module(leaves[0], leaves[0] if key is None else leaves[2], leaves[1], need_weights=False)
    assert weights is None
    names = ["out", "grad.x", "grad.value"] + ["grad.key"] * (key is not None) + [n for n, _ in module.named_parameters()]
    grads = torch.autograd.grad(out, leaves + list(module.parameters()), grad_out)
    return dict(zip(names, (out.detach(),) + grads))


def test_fused_module_matches_the_stock_module_in_float64_at_the_reference_shape():
    stock, fused = stock_and_fused(256, 8)
    x, value, _, go = make_inputs(300, 300, 1, 8, 32, torch.float64)
    want = module_results(stock, x, value, go)
    got = module_results(fused, x.float().to(DEV), value.float().to(DEV), go.float().to(DEV))
    for name in want:
        assert_close(got[name], want[name], TOL[F32], name)


def recorded_operator_calls(monkeypatch):
    """The keyword arguments of every call the module makes to the operator from here on."""
    from devis_amd.functions import self_attention
    calls, real = [], self_attention.multihead_attention
    monkeypatch.setattr(self_attention, "multihead_attention", lambda *a, **k: calls.append(k) or real(*a, **k))
    return calls


def test_fused_module_in_training_mode_matches_the_oracle_under_the_seed_it_drew(monkeypatch):
    """dropout = 0.5 in training mode at [33, 2, 64], 4 heads of 16: the module draws the seed, the test records the tensor it
    hands to the operator, restates the mask from it and compares with the float64 restatement of the module -- the stock
    projections around the oracle's attention with that mask -- output, input gradients and every parameter gradient."""
    import torch.nn.functional as F
    E, H, L, N, p = 64, 4, 33, 2, 0.5
    stock, fused = stock_and_fused(E, H, dropout=p)
    fused.train()
    x, value, _, go = (t.float().double() for t in make_inputs(L, L, N, H, E // H, torch.float64))
    calls = recorded_operator_calls(monkeypatch)
    got = module_results(fused, x.float().to(DEV), value.float().to(DEV), go.float().to(DEV))
    assert len(calls) == 1 and calls[0]["p"] == p
    seed = calls[0]["seed"]
    assert seed.dtype == torch.int64 and seed.numel() == 1 and seed.is_cuda
    keep = O.keep_mask(int(seed.item()), N, H, L, L, p)
    assert 0.4 < float(keep.double().mean()) < 0.6
    params = {name: t.detach().clone().requires_grad_(True) for name, t in stock.named_parameters()}
    xs, vs = x.requires_grad_(True), value.requires_grad_(True)
    weight, bias = params["in_proj_weight"], params["in_proj_bias"]
    q, k, v = (F.linear(t, weight[i * E:(i + 1) * E], bias[i * E:(i + 1) * E]) for i, t in enumerate((xs, xs, vs)))
    out = F.linear(O.attention(q, k, v, H, keep, O.scale_of(p)), params["out_proj.weight"], params["out_proj.bias"])
    grads = torch.autograd.grad(out, [xs, vs] + list(params.values()), go)
    want = dict(zip(["out", "grad.x", "grad.value"] + list(params), (out.detach(),) + grads))
    assert sorted(want) == sorted(got) and len(want) == 7
    for name in want:
        assert_close(got[name], want[name], TOL[F32], "training " + name)


def test_fused_module_matches_the_stock_module_with_a_separate_key_and_batch_first(monkeypatch):
    """Eval mode, [N, L, E] inputs, L = 21 queries on S = 50 keys, 2 heads of 48 (CT = 3): three projections, operands that are
    transposed views."""
    E, H, L, S, N = 96, 2, 21, 50, 2
    stock, fused = stock_and_fused(E, H, batch_first=True)
    x, key, value, go = (t.transpose(0, 1).contiguous() for t in make_inputs(L, S, N, H, E // H, torch.float64))
    assert tuple(x.shape) == (N, L, E) and tuple(key.shape) == (N, S, E)
    want = module_results(stock, x, value, go, key)
    calls = recorded_operator_calls(monkeypatch)
    got = module_results(fused, *(t.float().to(DEV) for t in (x, value, go, key)))
    assert len(calls) == 1 and calls[0]["p"] == 0.0 and sorted(want) == sorted(got) and len(want) == 8
    for name in want:
        assert_close(got[name], want[name], TOL[F32], "separate key, batch_first: " + name)


def decoder_case(device, dtype):
    case, module = LG.load_case("decoder"), LG.reference_module()
    layer, inputs, attention = LG.build_layer(module, "decoder", case, device, dtype)
    return case, module, layer, inputs, attention


def test_fused_module_matches_the_stock_module_on_the_decoder_fixture():
    case = LG.load_case("decoder")
    state = {k[len("state.self_attn."):]: v for k, v in case.items() if k.startswith("state.self_attn.")}
    stock, fused = stock_and_fused(LG.D_MODEL, LG.HEADS, state)
    x = (case["tgt"] + case["query_pos"]).transpose(0, 1)
    value, go = case["tgt"].transpose(0, 1), case["grad_out"].transpose(0, 1)
    assert tuple(x.shape) == (6, 1, 32)
    want = module_results(stock, x, value, go)
    got = module_results(fused, x.float().to(DEV), value.float().to(DEV), go.float().to(DEV))
    for name in want:
        assert_close(got[name], want[name], TOL[F32], name)


def test_the_patched_decoder_layer_reproduces_the_reference_fixture():
    import devis_amd
    case, module, layer, inputs, attention = decoder_case(DEV, F32)
    undo = devis_amd.patch_transformer_layers(module)
    previous = devis_amd.patch_self_attention(layer)
    try:
        assert type(layer.self_attn) is devis_amd.FusedMultiheadAttention
        out = layer(*inputs)
        params = dict(layer.named_parameters())
        grads = torch.autograd.grad(out, [inputs[0], attention] + list(params.values()), case["grad_out"].to(DEV, F32))
        got = {"out": out.detach(), "grad.tgt": grads[0], "grad.attention": grads[1]}
        got.update({"grad." + name: g for name, g in zip(params, grads[2:])})
        wanted = [k for k in case if k == "out" or k.startswith("grad.")]
        assert sorted(got) == sorted(wanted)
        for key in wanted:
            assert_close(got[key], case[key], 1e-4, key)
    finally:
        devis_amd.unpatch_self_attention(previous)
        devis_amd.unpatch_transformer_layers(module, undo)


def test_autocast_gives_the_dtypes_of_the_stock_module():
    """[300, 1, 256], 8 heads -- the reference's shape -- with the parameters nn.MultiheadAttention itself initialises.  The
    float64 stock module is fed what the autocast region consumes, the inputs and the parameters rounded to bfloat16, as every
    comparison here feeds the oracle the already rounded inputs; what is measured is the arithmetic in between.

    Why torch's own initialisation and not the unit-normal biases of the float32 tests: under autocast q and k reach the softmax
    rounded to bfloat16, so a logit s is off by about |s| * 2^-8 and its probability by that share, whatever computes the
    attention.  Unit-normal in_proj_bias triples |q| and |k| and with them the logits, and 1e-2 of float64 is then out of
    bfloat16's reach for ANY implementation: at [70, 2, 256] the gradient of in_proj_weight (its q rows) is off by 1.26e-2 of
    max|want| here, 1.32e-2 for stock nn.MultiheadAttention under the same autocast on the GPU and 1.40e-2 for it under CPU
    autocast; at [300, 1, 256] 1.98e-2 / 1.88e-2 / 2.10e-2.  A case the stock module fails tells nothing about this one.  With
    the module's own parameters bfloat16 is well inside the bar: every tensor within 4.6e-3 here, 5.6e-3 for stock (measured on
    an MI355X).  The 6-row decoder fixture (D = 4) is too small for a max-norm bound of 2.5 bfloat16 ulps to hold without
    averaging: 1.12e-2 here, 1.40e-2 for stock.  DESIGN.md section 20 keeps all of these figures."""
    import devis_amd
    stock, fused = stock_and_fused(256, 8, unit_biases=False)
    reference = nn.MultiheadAttention(256, 8).to(DEV).eval()
    reference.load_state_dict(stock.state_dict())
    with torch.no_grad():
        for param in stock.parameters():
            param.copy_(param.to(BF16))
    x, value, _, go = make_inputs(300, 300, 1, 8, 32, BF16)
    want = module_results(stock, x.double(), value.double(), go.double())
    xs, vs = x.float().to(DEV), value.float().to(DEV)
    with torch.autocast("cuda", dtype=BF16):
        theirs = module_results(reference, xs, vs, go.to(DEV))
        calls = []
        real = devis_amd.functions.self_attention._forward
        devis_amd.functions.self_attention._forward = lambda *a, **k: calls.append(a[0].dtype) or real(*a, **k)
        try:
            mine = module_results(fused, xs, vs, go.to(DEV))
        finally:
            devis_amd.functions.self_attention._forward = real
    assert calls == [BF16]
    missed = []
    for name in want:
        assert mine[name].dtype == theirs[name].dtype == (BF16 if name == "out" else F32), name
        ref = float(want[name].abs().max())
        err, stock_err = (float((r[name].double().cpu() - want[name]).abs().max()) / ref for r in (mine, theirs))
        print("autocast %s: max error %.3e of max |want|, the stock module's %.3e (tol %.0e)" % (name, err, stock_err, TOL[BF16]))
        if err > TOL[BF16]:
            missed.append((name, err, stock_err))
    assert not missed, missed
