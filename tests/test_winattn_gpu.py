"""GPU tests of the Swin backbone's window-attention kernels (include/winattn.h) against the float64 oracle of
tests/winattn_oracle.py on the same rounded inputs: the output and both gradients at every shape case, 16-bit storage beside a
float32 table, a view that is not 16-byte aligned, the bitwise properties, a peaked softmax, the patched stage against the
fixture recorded from the reference, and results allocated over stale memory.

Tolerance: max|got - want| <= tol * max|want| per tensor (tests/test_attmap_gpu.py::assert_close), tol = 1e-4 for a float32
and 1e-2 for a 16-bit storage dtype.  Plain float32 torch in this formulation deviates from float64 by at most 5.4e-7 of
max|want| at these shape classes, so the float32 bar leaves a margin of more than a hundredfold."""
import pytest
import torch

import stale_memory
import winattn_cases as C
import winattn_oracle as O
from test_attmap_gpu import TOL, assert_close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAMES = ("out", "grad_qkv", "grad_bias_table")


def run(qkv, table, go, H, ws, shift, wants=(True, True)):
    """(out, grad_qkv, grad_bias_table) of the operator on GPU tensors, passed as the views they are; None where not wanted."""
    import devis_amd
    a, b = qkv.detach().requires_grad_(wants[0]), table.detach().requires_grad_(wants[1])
    out = devis_amd.window_attention(a, b, H, ws, shift)
    grads = list(torch.autograd.grad(out, [t for t, w in zip((a, b), wants) if w], go))
    return (out.detach(),) + tuple(grads.pop(0) if w else None for w in wants)


def check(case, dtype=F32, table_dtype=None, gain=1.0, what=""):
    ws, shift, Hp, Wp, B, H, D = case
    qkv, table, go = C.make_inputs(case, dtype, table_dtype, gain=gain)
    want = O.attention_grads(qkv, table, H, ws, shift, go)
    got = run(qkv.to(DEV), table.to(DEV), go.to(DEV), H, ws, shift)
    for name, a, b, like in zip(NAMES, got, want, (go, qkv, table)):
        assert a.dtype == like.dtype and a.shape == b.shape and a.is_contiguous() and bool(a.isfinite().all()), name
        assert_close(a, b, TOL[dtype], "%s %s %s" % (what or C.case_id(case), dtype, name))
    return got


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def on_gpu(case, dtype=F32, table_dtype=None, seed=0):
    return tuple(t.to(DEV) for t in C.make_inputs(case, dtype, table_dtype, seed=seed))


# ---- oracle parity -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", C.SHAPES + C.UNSHIFTED + [C.CHUNKED], ids=C.case_id)
def test_float32_matches_the_oracle(case):
    check(case)


@pytest.mark.parametrize("wide", [True, False], ids=["float32 table", "16-bit table"])
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("case", C.SHAPES_16, ids=C.case_id)
def test_16_bit_operands_match_the_oracle(case, dtype, wide):
    check(case, dtype, F32 if wide else dtype)


def test_large_logits_stay_within_the_bound():
    check(C.SHAPES[3], gain=30.0, what="queries x 30")


# ---- bits ------------------------------------------------------------------------------------------------------------------------

def shifted(t, elements=1):
    """A dense view with t's values whose first element is ``elements`` elements past a 256-byte boundary."""
    base = torch.empty(t.numel() + 256, dtype=t.dtype, device=t.device)
    view = base[elements:elements + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("case", [C.SHAPES[3], C.SHAPES[2], C.SHAPES[6]], ids=C.case_id)
def test_a_view_that_is_not_16_byte_aligned_gives_the_bits_of_the_aligned_run(case, dtype):
    ws, shift, Hp, Wp, B, H, D = case
    qkv, table, go = on_gpu(case, dtype, F32)
    assert qkv.data_ptr() % 16 == 0 and go.data_ptr() % 16 == 0
    aligned = run(qkv, table, go, H, ws, shift)
    for views in ((shifted(qkv), table, go), (qkv, table, shifted(go)), (shifted(qkv), shifted(table), shifted(go, 3))):
        got = run(*views, H, ws, shift)
        assert all(same_bits(a, b) for a, b in zip(got, aligned))


def test_results_are_bitwise_reproducible_and_independent_of_the_batch():
    case = C.SHAPES[3]
    ws, shift, Hp, Wp, B, H, D = case
    qkv, table, go = on_gpu(case)
    first, again = run(qkv, table, go, H, ws, shift), run(qkv, table, go, H, ws, shift)
    assert all(same_bits(a, b) for a, b in zip(first, again))
    # an image alone against the same image in the batch
    for b in range(B):
        alone = run(qkv[b:b + 1].clone(), table, go[b:b + 1].clone(), H, ws, shift)
        assert same_bits(alone[0], first[0][b:b + 1]) and same_bits(alone[1], first[1][b:b + 1])
    # each gradient alone against the full backward
    only_qkv = run(qkv, table, go, H, ws, shift, (True, False))
    only_table = run(qkv, table, go, H, ws, shift, (False, True))
    assert only_qkv[2] is None and only_table[1] is None
    assert same_bits(only_qkv[0], first[0]) and same_bits(only_qkv[1], first[1]) and same_bits(only_table[2], first[2])
    # without autograd: the same out
    import devis_amd
    with torch.no_grad():
        assert same_bits(devis_amd.window_attention(qkv, table, H, ws, shift), first[0])


def test_chunked_table_gradient_is_reproducible():
    ws, shift, Hp, Wp, B, H, D = C.CHUNKED
    qkv, table, go = on_gpu(C.CHUNKED)
    first, again = run(qkv, table, go, H, ws, shift), run(qkv, table, go, H, ws, shift)
    assert all(same_bits(a, b) for a, b in zip(first, again))


# ---- stale memory ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF16])
def test_results_over_stale_memory_are_complete_and_stay_inside(monkeypatch, dtype):
    """Outputs, lse, out_acc, both gradients and the workspace are handed out holding NaN payloads between guard zones: every
    element is written before it is read, and nothing outside is touched."""
    from devis_amd.functions import window_attention
    for case in (C.SHAPES[3], C.SHAPES[2], C.CHUNKED):
        ws, shift, Hp, Wp, B, H, D = case
        qkv, table, go = on_gpu(case, dtype, F32)
        clean = run(qkv, table, go, H, ws, shift)
        with monkeypatch.context() as m:
            shim = stale_memory.install(m, [window_attention])
            got = run(qkv, table, go, H, ws, shift)
            assert len(shim.buffers) == (5 if dtype == F32 else 6) and shim.guards_intact()
        assert all(bool(t.isfinite().all()) for t in got) and all(same_bits(a, b) for a, b in zip(got, clean))


# ---- the block -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_checkpoint", [False, True])
def test_patched_stage_reproduces_the_fixture_on_the_gpu(monkeypatch, use_checkpoint):
    import devis_amd
    from devis_amd import _winattn
    case = C.load_fixture()
    layer, x = C.build_layer(case, F32, DEV, use_checkpoint=use_checkpoint)
    layer.train(use_checkpoint)                              # (every drop rate is 0)
    calls, forward, backward = [], _winattn.forward, _winattn.backward
    monkeypatch.setattr(_winattn, "forward", lambda *a: calls.append("forward") or forward(*a))
    monkeypatch.setattr(_winattn, "backward", lambda *a: calls.append("backward") or backward(*a))
    previous = devis_amd.patch_window_attention(C)
    try:
        got = C.run_layer(layer, x, case)
    finally:
        devis_amd.unpatch_window_attention(C, previous)
    assert calls.count("forward") == (4 if use_checkpoint else 2) and calls.count("backward") == 2
    assert sorted(got) == sorted(k for k in case if k == "out" or k.startswith("grad."))
    for key in sorted(got):
        assert_close(got[key], case[key], TOL[F32], key)


def test_patched_block_under_autocast_takes_the_float32_table(monkeypatch):
    import devis_amd
    from devis_amd import _winattn
    torch.manual_seed(7)
    blk = C.SwinTransformerBlock(64, 2, window_size=7, shift_size=3).to(DEV).eval()
    blk.H, blk.W = 12, 17
    x = torch.randn(2, 12 * 17, 64, device=DEV)
    mask = O.sliced_mask(14, 21, 7, 3).to(DEV, F32)
    seen, forward = [], _winattn.forward
    monkeypatch.setattr(_winattn, "forward", lambda code, wide, qkv, table, *a: seen.append((wide, qkv.dtype, table.dtype)) or forward(code, wide, qkv, table, *a))
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        want = blk(x, mask)
        previous = devis_amd.patch_window_attention(C)
        try:
            got = blk(x, None)
        finally:
            devis_amd.unpatch_window_attention(C, previous)
    assert seen == [(True, BF16, F32)] and got.dtype == want.dtype and got.shape == want.shape and bool(got.isfinite().all())
