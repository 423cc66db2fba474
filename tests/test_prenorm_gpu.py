"""GPU tests of the Swin glue kernels (include/prenorm.h) against the float64 oracle of tests/prenorm_oracle.py on the same
rounded inputs: the three source forms and both destinations with every gradient at the channel counts, maps and merges where
the kernels change path, the drop-path scale, column sums over several chunks, every accepted dtype mix, the bitwise
properties, results allocated over stale memory, and the patched stage against the fixture recorded from the reference.

Tolerance: max|got - want| <= tol * max|want| per tensor (tests/test_attmap_gpu.py::assert_close), tol = 1e-4 for a float32
and 1e-2 for a 16-bit result.  Plain float32 torch in this formulation (F.layer_norm, F.pad, slices and cat, by autograd, on the
CPU) deviates from float64 by at most 2.0e-7 of max|want| at these shapes (grad_weight; 1.7e-7 for y), so the float32 bar
leaves a margin of five hundredfold."""
import numpy as np
import pytest
import torch

import prenorm_oracle as O
import stale_memory
import swinglue_cases as S
from test_attmap_gpu import TOL, assert_close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
CHANNELS = [4, 6, 256, 260, 1536, 3072]     # a quad and 63 idle lanes; per element; one group; a group tail; 8 groups; the limit
MAPS = [(6, 9, 4), (8, 8, 4), (1, 1, 7)]    # padding on both sides; none; a 7 x 7 map that is almost all padding
MERGES = [(5, 7, 16), (6, 9, 16), (4, 4, 4), (1, 1, 4), (3, 3, 6), (4, 6, 768)]
KEEPS = {"mixed": [0.0, 1 / 0.7, 1 / 0.7], "all zero": [0.0, 0.0, 0.0], "none": None}
NAMES = ("s", "y", "grad_x", "grad_delta", "grad_weight", "grad_bias")


def rand(*shape, seed, dtype=F32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def norm_inputs(B, L, C, map_size=None, dtypes=(F32, F32, F32, F32), seed=0):
    """{x, delta, weight, bias, grad_y, grad_s} on the CPU, rounded to (x, delta, y, parameter) dtypes."""
    tx, td, ty, tp = dtypes
    y_shape = (B, map_size[2], map_size[3], C) if map_size else (B, L, C)
    return {"x": rand(B, L, C, seed=seed + 1, dtype=tx), "delta": rand(B, L, C, seed=seed + 2, dtype=td),
            "weight": (rand(C, seed=seed + 3) + 1).to(tp), "bias": rand(C, seed=seed + 4, dtype=tp),
            "grad_y": rand(*y_shape, seed=seed + 5, dtype=ty), "grad_s": rand(B, L, C, seed=seed + 6, dtype=tx)}


def merge_inputs(B, H, W, C, dtypes=(F32, F32, F32), seed=0):
    tx, ty, tp = dtypes
    rows = ((H + 1) // 2) * ((W + 1) // 2)
    return {"x": rand(B, H * W, C, seed=seed + 1, dtype=tx), "weight": (rand(4 * C, seed=seed + 3) + 1).to(tp),
            "bias": rand(4 * C, seed=seed + 4, dtype=tp), "grad_y": rand(B, rows, 4 * C, seed=seed + 5, dtype=ty)}


def on_gpu(d):
    return {k: v.to(DEV) for k, v in d.items()}


def run_norm(d, residual=True, keep=None, map_size=None, out_dtype=None, wants=(True, True, True, True), use_s=True):
    """{s, y, grad_x, grad_delta, grad_weight, grad_bias} of the operator on GPU tensors, passed as the views they are."""
    import devis_amd
    leaves = [d[k].detach().requires_grad_(w) for k, w in zip(("x", "delta", "weight", "bias"), wants)]
    if not residual:
        leaves[1] = None
    s, y = devis_amd.residual_layer_norm(*leaves, keep=keep, map_size=map_size, out_dtype=out_dtype)
    wanted = [t for t in leaves if t is not None and t.requires_grad]
    outs, gouts = ([s, y], [d["grad_s"], d["grad_y"]]) if residual and use_s else ([y], [d["grad_y"]])
    grads = list(torch.autograd.grad(outs, wanted, gouts)) if wanted else []
    got = {"s": s.detach() if residual else None, "y": y.detach()}
    for name, leaf in zip(NAMES[2:], leaves):
        got[name] = grads.pop(0) if leaf is not None and leaf.requires_grad else None
    return got


def run_merge(d, H, W, out_dtype=None):
    import devis_amd
    leaves = [d[k].detach().requires_grad_(True) for k in ("x", "weight", "bias")]
    y = devis_amd.patch_merge_norm(leaves[0], H, W, leaves[1], leaves[2], out_dtype=out_dtype)
    gx, gw, gb = torch.autograd.grad(y, leaves, d["grad_y"])
    return {"y": y.detach(), "grad_x": gx, "grad_weight": gw, "grad_bias": gb}


def want_norm(d, residual=True, keep=None, map_size=None, use_s=True):
    delta = d["delta"] if residual else None
    s_dtype = d["x"].dtype if d["x"].dtype != F32 else None
    want = O.forward(d["x"], delta, d["weight"], d["bias"], 1e-5, keep, None, map_size, s_dtype)
    want.update(O.grads(d["x"], delta, d["weight"], d["bias"], 1e-5, d["grad_y"], d["grad_s"] if residual and use_s else None, keep,
                        None, map_size, s_dtype))
    return want


def compare(got, want, what):
    for name in got:
        a, b = got[name], want[name]
        if a is None:
            continue
        assert a.is_contiguous() and bool(a.isfinite().all()), (what, name)
        assert_close(a, b.reshape(a.shape), TOL[a.dtype], "%s %s %s" % (what, a.dtype, name))


def check_norm(B, L, C, residual=True, keep=None, map_size=None, dtypes=(F32, F32, F32, F32), what=""):
    d = norm_inputs(B, L, C, map_size, dtypes)
    keep_t = None if keep is None else torch.tensor(keep, dtype=F32)
    got = run_norm(on_gpu(d), residual, None if keep is None else keep_t.to(DEV), map_size, dtypes[2] if dtypes[2] != dtypes[0] else None)
    assert got["y"].dtype == dtypes[2] and (not residual or (got["s"].dtype == dtypes[0] and got["grad_delta"].dtype == dtypes[1]))
    assert got["grad_x"].dtype == dtypes[0] and got["grad_weight"].dtype == got["grad_bias"].dtype == dtypes[3]
    compare(got, want_norm(d, residual, keep_t, map_size), what or "C=%d" % C)
    return got


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def all_same_bits(got, want):
    return all((got[k] is None and want[k] is None) or same_bits(got[k], want[k]) for k in want)


# ---- oracle parity -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("C", CHANNELS)
def test_float32_tokens_match_the_oracle(C, residual):
    """B = 2 with 54 tokens: 108 rows, so the column sums combine four chunks, the last of 12 rows."""
    from devis_amd import _prenorm
    assert -(-108 // _prenorm.tile()) >= 3 and 108 % _prenorm.tile()
    check_norm(2, 54, C, residual)


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("H,W,ws", MAPS)
def test_float32_maps_match_the_oracle_and_pad_with_zeros(H, W, ws, residual):
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    for C in (16, 6):
        got = check_norm(2, H * W, C, residual, None, (H, W, Hp, Wp), what="map %dx%d in %dx%d C=%d" % (H, W, Hp, Wp, C))
        pad = got["y"].clone()
        pad[:, :H, :W] = 0
        assert tuple(pad.shape) == (2, Hp, Wp, C) and not bool(pad.view(torch.int32).any())        # exactly +0.0


@pytest.mark.parametrize("H,W,C", MERGES)
def test_float32_merges_match_the_oracle(H, W, C):
    d = merge_inputs(2, H, W, C)
    want = O.forward(d["x"], None, d["weight"], d["bias"], 1e-5, merge=(H, W))
    want.update(O.grads(d["x"], None, d["weight"], d["bias"], 1e-5, d["grad_y"], merge=(H, W)))
    compare(run_merge(on_gpu(d), H, W), want, "merge %dx%dx%d" % (H, W, C))


@pytest.mark.parametrize("keep", list(KEEPS), ids=list(KEEPS))
def test_keep_scales_delta_per_batch_entry(keep):
    for map_size in (None, (6, 9, 8, 12)):
        check_norm(3, 54, 260, True, KEEPS[keep], map_size, what="keep %s" % keep)


def test_one_chunk_is_one_call_without_a_workspace(monkeypatch):
    from devis_amd import _prenorm
    tile = _prenorm.tile()
    calls, forward, backward = [], _prenorm.forward, _prenorm.backward
    monkeypatch.setattr(_prenorm, "forward", lambda *a: calls.append("forward") or forward(*a))
    monkeypatch.setattr(_prenorm, "backward", lambda *a: calls.append(("backward", a[9] is not None)) or backward(*a))
    check_norm(1, tile, 260, what="one chunk")
    check_norm(1, tile + 1, 260, what="two chunks")
    assert calls == ["forward", ("backward", False), "forward", ("backward", True)]
    assert _prenorm.workspace_bytes(_prenorm.Shape(1, 1, tile, 260, 0, 0, 1, 0)) == 0


MIXES = [(F32, F32, F32, F32)] + [m for h in (BF16, F16) for m in (
    (h, h, h, h), (h, h, h, F32), (F32, h, F32, F32), (F32, F32, h, F32), (F32, h, h, F32))]


@pytest.mark.parametrize("dtypes", MIXES, ids=lambda m: "-".join(str(t).split(".")[1] for t in m))
def test_every_accepted_dtype_mix_matches_the_oracle(dtypes):
    check_norm(2, 54, 256, True, None, None, dtypes)
    check_norm(2, 54, 256, True, None, (6, 9, 8, 12), dtypes, what="map")
    if dtypes[1] == dtypes[0]:                                # (no delta: the plain form and the merge)
        check_norm(2, 54, 256, False, None, None, dtypes, what="plain")
        H, W, C = MERGES[0]
        d = merge_inputs(2, H, W, C, (dtypes[0], dtypes[2], dtypes[3]))
        want = O.forward(d["x"], None, d["weight"], d["bias"], 1e-5, merge=(H, W))
        want.update(O.grads(d["x"], None, d["weight"], d["bias"], 1e-5, d["grad_y"], merge=(H, W)))
        got = run_merge(on_gpu(d), H, W, dtypes[2] if dtypes[2] != dtypes[0] else None)
        assert got["y"].dtype == dtypes[2] and got["grad_x"].dtype == dtypes[0] and got["grad_weight"].dtype == dtypes[3]
        compare(got, want, "merge")


def test_unsupported_mixes_take_the_composite_on_the_gpu(monkeypatch):
    import devis_amd
    from devis_amd import _prenorm
    monkeypatch.setattr(_prenorm, "forward", lambda *a: pytest.fail("a kernel call"))
    x = torch.randn(2, 5, 8, device=DEV, dtype=torch.float64)
    s, y = devis_amd.residual_layer_norm(x, x, torch.ones(8, device=DEV, dtype=torch.float64), torch.zeros(8, device=DEV, dtype=torch.float64))
    assert y.dtype == torch.float64 and bool(y.isfinite().all())
    wide = torch.randn(1, 2, 3076, device=DEV)
    assert devis_amd.residual_layer_norm(wide, None, torch.ones(3076, device=DEV), torch.zeros(3076, device=DEV))[1].shape == wide.shape


# ---- bits ------------------------------------------------------------------------------------------------------------------------

def shifted(t, elements=1):
    """A dense view with t's values whose first element is ``elements`` elements past a 256-byte boundary."""
    base = torch.empty(t.numel() + 256, dtype=t.dtype, device=t.device)
    view = base[elements:elements + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def test_results_are_bitwise_reproducible_and_independent_of_the_batch():
    keep = torch.tensor([0.0, 1 / 0.7, 1 / 0.7], device=DEV)
    for C, map_size in ((260, None), (16, (6, 9, 8, 12)), (1536, None)):
        d = on_gpu(norm_inputs(3, 54, C, map_size))
        first, again = run_norm(d, True, keep, map_size), run_norm(d, True, keep, map_size)
        assert all_same_bits(again, first)
        for b in range(3):
            alone = run_norm({k: (v[b:b + 1].clone() if v.dim() > 1 else v) for k, v in d.items()}, True, keep[b:b + 1].clone(), map_size)
            for name in ("y", "s", "grad_x", "grad_delta"):
                assert same_bits(alone[name], first[name][b:b + 1]), (C, b, name)
        # each gradient alone against the full backward; without autograd: the same s and y
        for i, name in enumerate(NAMES[2:]):
            only = run_norm(d, True, keep, map_size, wants=tuple(j == i for j in range(4)))
            assert same_bits(only[name], first[name]) and sum(only[n] is not None for n in NAMES[2:]) == 1, name
        import devis_amd
        with torch.no_grad():
            s, y = devis_amd.residual_layer_norm(d["x"], d["delta"], d["weight"], d["bias"], keep=keep, map_size=map_size)
        assert same_bits(s, first["s"]) and same_bits(y, first["y"])
    H, W, C = MERGES[0]
    d = on_gpu(merge_inputs(3, H, W, C))
    first, again = run_merge(d, H, W), run_merge(d, H, W)
    assert all_same_bits(again, first)
    for b in range(3):
        alone = run_merge({k: (v[b:b + 1].clone() if v.dim() > 1 else v) for k, v in d.items()}, H, W)
        assert same_bits(alone["y"], first["y"][b:b + 1]) and same_bits(alone["grad_x"], first["grad_x"][b:b + 1])


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_operands_that_are_not_16_byte_aligned_give_the_bits_of_the_aligned_run(dtype):
    mix = (dtype, dtype, dtype, F32)
    for C, map_size in ((256, None), (16, (6, 9, 8, 12)), (3072, None)):
        d = on_gpu(norm_inputs(2, 54, C, map_size, mix))
        assert all(v.data_ptr() % 16 == 0 for v in d.values())
        aligned = run_norm(d, map_size=map_size)
        for names in (("x",), ("delta",), ("weight", "bias"), ("grad_y",), ("grad_s",), tuple(d)):
            views = {k: (shifted(v, 1 if k != "grad_y" else 3) if k in names else v) for k, v in d.items()}
            assert all_same_bits(run_norm(views, map_size=map_size), aligned), (C, names)
    for H, W, C in (MERGES[1], MERGES[5]):
        d = on_gpu(merge_inputs(2, H, W, C, (dtype, dtype, F32)))
        aligned = run_merge(d, H, W)
        for names in (("x",), ("grad_y",), tuple(d)):
            views = {k: (shifted(v) if k in names else v) for k, v in d.items()}
            assert all_same_bits(run_merge(views, H, W), aligned), (H, W, C, names)


def test_a_16_bit_y_is_the_float32_y_rounded_once():
    for half in (BF16, F16):
        d = on_gpu(norm_inputs(2, 54, 260))
        import devis_amd
        with torch.no_grad():
            _, y32 = devis_amd.residual_layer_norm(d["x"], d["delta"], d["weight"], d["bias"])
            _, y16 = devis_amd.residual_layer_norm(d["x"], d["delta"], d["weight"], d["bias"], out_dtype=half)
            _, m32 = devis_amd.residual_layer_norm(d["x"], None, d["weight"], d["bias"], map_size=(6, 9, 8, 12))
            _, m16 = devis_amd.residual_layer_norm(d["x"], None, d["weight"], d["bias"], map_size=(6, 9, 8, 12), out_dtype=half)
        assert same_bits(y32.to(half), y16) and same_bits(m32.to(half), m16)


def test_the_mean_has_the_bits_of_the_headers_order():
    from devis_amd.functions import pre_norm
    for C in (6, 260, 1536):
        d = on_gpu(norm_inputs(2, 54, C))
        s, y, mean, rstd = pre_norm._forward(d["x"], None, d["weight"], d["bias"], None, 1e-5, None, None)
        want = O.mean_f32(d["x"].cpu().numpy().reshape(-1, C))
        assert np.array_equal(mean.cpu().numpy().reshape(-1).view(np.uint32), want.view(np.uint32)), C


def test_rows_with_keep_zero_take_exactly_x():
    d = on_gpu(norm_inputs(3, 54, 260))
    d["x"][0, 0, :4] = torch.tensor([-0.0, 0.0, -1.5, 3.0], device=DEV)
    d["delta"][0] = float("inf")
    d["delta"][0, ::2] = float("nan")
    keep = torch.tensor([0.0, 1 / 0.7, 1 / 0.7], device=DEV)
    for map_size in (None, (6, 9, 8, 12)):
        if map_size is not None:
            d["grad_y"] = torch.randn(3, 8, 12, 260, device=DEV)
        got = run_norm(d, True, keep, map_size)
        assert same_bits(got["s"][0], d["x"][0])
        assert not bool(got["grad_delta"][0].view(torch.int32).any())                  # exactly 0
        assert all(bool(got[n].isfinite().all()) for n in ("y", "grad_x", "grad_weight", "grad_bias"))
        assert bool(got["s"][1:].isfinite().all()) and bool(got["grad_delta"][1:].isfinite().all())


# ---- stale memory ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF16])
def test_results_over_stale_memory_are_complete_and_stay_inside(monkeypatch, dtype):
    """Outputs, statistics, gradients and the workspace are handed out holding NaN payloads between guard zones: every element
    is written before it is read, a map's padding is exactly 0, and nothing outside is touched."""
    from devis_amd.functions import pre_norm
    mix = (dtype, dtype, dtype, F32)
    keep = torch.tensor([0.0, 2.0], device=DEV)
    for C, H, W, Hp, Wp in ((16, 6, 9, 8, 12), (6, 1, 1, 7, 7), (260, 6, 9, 8, 12)):
        d = on_gpu(norm_inputs(2, H * W, C, (H, W, Hp, Wp), mix))
        clean = run_norm(d, True, keep, (H, W, Hp, Wp))
        with monkeypatch.context() as m:
            shim = stale_memory.install(m, [pre_norm])
            got = run_norm(d, True, keep, (H, W, Hp, Wp))
            assert len(shim.buffers) >= 8 and shim.guards_intact()
        assert all(bool(t.isfinite().all()) for t in got.values()) and all_same_bits(got, clean)
        pad = got["y"].clone()
        pad[:, :H, :W] = 0
        assert not bool(pad.view(torch.int16 if dtype == BF16 else torch.int32).any())
    for H, W, C in (MERGES[0], MERGES[3], MERGES[4]):       # odd H and W: every element of grad_x is written
        d = on_gpu(merge_inputs(2, H, W, C, (dtype, dtype, F32)))
        clean = run_merge(d, H, W)
        with monkeypatch.context() as m:
            shim = stale_memory.install(m, [pre_norm])
            got = run_merge(d, H, W)
            assert len(shim.buffers) >= 6 and shim.guards_intact()
        assert all(bool(t.isfinite().all()) for t in got.values()) and all_same_bits(got, clean)


# ---- the stage -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_checkpoint", [False, True])
def test_patched_stage_reproduces_the_fixture_on_the_gpu(monkeypatch, use_checkpoint):
    import devis_amd
    from devis_amd import _prenorm
    case = S.load_fixture()
    layer, x = S.build_layer(case, F32, DEV, use_checkpoint=use_checkpoint)
    layer.train(use_checkpoint)                              # (every drop rate is 0)
    calls, forward, backward = [], _prenorm.forward, _prenorm.backward
    monkeypatch.setattr(_prenorm, "forward", lambda *a: calls.append("forward") or forward(*a))
    monkeypatch.setattr(_prenorm, "backward", lambda *a: calls.append("backward") or backward(*a))
    masks = S.BasicLayer.built_masks
    previous = devis_amd.patch_swin_glue(S)
    try:
        got = S.run_layer(layer, x, case)
    finally:
        devis_amd.unpatch_swin_glue(S, previous)
    assert calls.count("forward") == (9 if use_checkpoint else 5) and calls.count("backward") == 5
    assert S.BasicLayer.built_masks == masks
    assert sorted(got) == sorted(k for k in case if k in ("x_out", "x_down") or k.startswith("grad."))
    for key in sorted(got):
        assert_close(got[key], case[key], TOL[F32], key)


def test_patched_stage_in_training_with_drop_path_matches_the_stock_stage():
    import devis_amd
    layer, x = S.build_layer(None, F32, DEV, drop_path=0.3)
    layer.train()
    B, H, W = S.LAYER_INPUT
    go, gd = torch.randn(B, H * W, 16, device=DEV), torch.randn(B, 20, 32, device=DEV)
    params = dict(layer.named_parameters())

    def run(seed):
        torch.manual_seed(seed)
        out = layer(x, H, W)
        return [out[0].detach(), out[3].detach()] + list(torch.autograd.grad([out[0], out[3]], [x] + list(params.values()), [go, gd]))

    seeds = (11, 12, 13, 14)
    want = [run(seed) for seed in seeds]
    previous = devis_amd.patch_swin_glue(S)
    try:
        got = [run(seed) for seed in seeds]
    finally:
        devis_amd.unpatch_swin_glue(S, previous)
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(want, want[1:]))              # the seeds draw different masks
    for seed, a, b in zip(seeds, got, want):
        for name, t, u in zip(["x_out", "x_down", "grad.x"] + ["grad." + n for n in params], a, b):
            assert_close(t, u.double().cpu(), TOL[F32], "seed %d %s" % (seed, name))


def test_patched_block_under_autocast_writes_16_bit_norms_beside_the_float32_stream(monkeypatch):
    import devis_amd
    from devis_amd import _prenorm
    torch.manual_seed(7)
    layer = S.BasicLayer(64, 2, 2, window_size=7, downsample=S.PatchMerging).to(DEV).eval()
    x = torch.randn(2, 12 * 17, 64, device=DEV)
    seen, forward = [], _prenorm.forward
    monkeypatch.setattr(_prenorm, "forward", lambda types, *a: seen.append((types.x, types.delta, types.y, types.param)) or forward(types, *a))
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        want = layer(x, 12, 17)
        previous = devis_amd.patch_swin_glue(S)
        try:
            got = layer(x, 12, 17)
        finally:
            devis_amd.unpatch_swin_glue(S, previous)
    assert seen == [(0, 0, 2, 0), (0, 2, 2, 0), (0, 2, 2, 0), (0, 2, 2, 0), (0, 0, 2, 0)]
    for a, b in ((got[0], want[0]), (got[3], want[3])):
        assert a.dtype == b.dtype and a.shape == b.shape and bool(a.isfinite().all())
