"""GPU tests of the two ends of the Swin backbone (include/swinends.h): ``devis_amd.patch_embed_norm`` and
``devis_amd.layer_norm_to_map`` against the float64 oracle restated from the header (tests/swinends_oracle.py), their bitwise
properties, results allocated over stale memory, and the patched stand-in backbone against the fixture recorded from the
reference.

The bars are the project's (tests/test_attmap_gpu.py::assert_close): ``max|got - want| <= tol * max|want|`` per tensor with
``tol = 1e-4`` for a float32 result and ``1e-2`` for a 16-bit one.  Plain float32 torch in these two formulations, measured on the
CPU over the shapes below against float64, deviates by at most 3.5e-7 of ``max|want|`` for the embedding (in
``grad_proj_bias``) and by at most 8.1e-7 for the output norm (in ``grad_bias`` at 2 x 67 x 70 x 192): the float32 bar leaves a
margin of more than a hundredfold.
"""
import functools

import pytest
import torch

import stale_memory
import swinends_oracle as O
from test_attmap_gpu import TOL, assert_close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
IMAGES = [(3, 10, 13, 4), (3, 8, 8, 4), (3, 3, 5, 4), (1, 5, 7, 2)]     # Cin, H, W, p: both axes padded and rows that are no
                                                                        # 16-byte multiples; no padding; one token row, mostly
                                                                        # padding; one channel and a 2 x 2 patch
EMBED_CHANNELS = [4, 6, 96, 192, 260, 1024]     # a quad; per element; the configurations'; a group tail; the limit
MAP_CHANNELS = [4, 6, 96, 260, 1536, 3072]
EMBED_GRADS = ("grad_proj_weight", "grad_proj_bias", "grad_norm_weight", "grad_norm_bias")
MAP_GRADS = ("grad_x", "grad_weight", "grad_bias")


def rand(*shape, seed, dtype=F32, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) + shift).to(dtype)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def all_same_bits(got, want):
    return all((got[k] is None and want[k] is None) or same_bits(got[k], want[k]) for k in want)


def shifted(t, nbytes=4):
    """A dense view with t's values whose first element is ``nbytes`` bytes past a 256-byte boundary."""
    elements = nbytes // t.element_size()
    base = torch.empty(t.numel() + 256, dtype=t.dtype, device=t.device)
    view = base[elements:elements + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


# ---- patch_embed_norm --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def embed_case(B, Cin, H, W, p, C, mix=(F32, F32), norm=True, bias=True):
    """(inputs on the CPU, rounded to their storage dtypes; the oracle's results).  ``mix`` = (image and parameters, tokens)."""
    dt, ydt = mix
    L = (-(-H // p)) * (-(-W // p))
    d = {"image": rand(B, Cin, H, W, seed=1, dtype=dt), "proj_weight": (rand(C, Cin, p, p, seed=2) / (Cin * p * p) ** 0.5).to(dt),
         "proj_bias": rand(C, seed=3, dtype=dt) if bias else None,
         "norm_weight": rand(C, seed=4, dtype=dt, shift=1.0) if norm else None, "norm_bias": rand(C, seed=5, dtype=dt) if norm else None,
         "grad_tokens": rand(B, L, C, seed=6, dtype=ydt)}
    want = O.embed_forward(d["image"], d["proj_weight"], d["proj_bias"], d["norm_weight"], d["norm_bias"])
    want.update(O.embed_grads(d["image"], d["proj_weight"], d["proj_bias"], d["norm_weight"], 1e-5, d["grad_tokens"]))
    return d, want


def run_embed(d, out_dtype=None, wants=(True, True, True, True)):
    """{tokens, grad_*} of the operator on GPU tensors, passed as the views they are."""
    import devis_amd
    names = ("proj_weight", "proj_bias", "norm_weight", "norm_bias")
    leaves = {k: (None if d[k] is None else d[k].detach().requires_grad_(w)) for k, w in zip(names, wants)}
    tokens = devis_amd.patch_embed_norm(d["image"], *(leaves[k] for k in names), out_dtype=out_dtype)
    asked = [k for k in names if leaves[k] is not None and leaves[k].requires_grad]
    grads = dict(zip(asked, torch.autograd.grad(tokens, [leaves[k] for k in asked], d["grad_tokens"]))) if asked else {}
    got = {"tokens": tokens.detach()}
    got.update({"grad_" + k: grads.get(k) for k in names})
    return got


def on_gpu(d):
    return {k: (None if v is None else v.to(DEV)) for k, v in d.items()}


def check_embed(*case, what=""):
    d, want = embed_case(*case)
    mix = case[6] if len(case) > 6 else (F32, F32)
    got = run_embed(on_gpu(d), out_dtype=mix[1])
    assert got["tokens"].dtype == mix[1] and got["tokens"].is_contiguous()
    assert_close(got["tokens"], want["tokens"], TOL[mix[1]], "embed %s tokens %s" % (what, case[:6]))
    for name in EMBED_GRADS:
        if want[name] is None or got[name] is None:
            assert got[name] is None and (want[name] is None or d[name[5:]] is None), name
            continue
        assert got[name].dtype == mix[0]
        assert_close(got[name], want[name], TOL[mix[0]], "embed %s %s %s" % (what, name, case[:6]))


@pytest.mark.parametrize("C", EMBED_CHANNELS)
def test_embedding_matches_the_oracle_at_every_channel_count(C):
    check_embed(3, 3, 10, 13, 4, C)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("image", IMAGES, ids=lambda i: "x".join(map(str, i)))
def test_embedding_matches_the_oracle_on_padded_and_unpadded_images(image, B):
    check_embed(B, *image, 96)
    check_embed(B, *image, 6)


def test_embedding_sums_of_one_chunk_and_of_two_chunks_plus_three_rows():
    from devis_amd import _swinends
    chunk, tile = _swinends.tile(_swinends.TILE_EMBED_CHUNK), _swinends.tile(_swinends.TILE_TOKENS)
    assert chunk % tile == 0
    check_embed(1, 1, 2 * (chunk // tile), 2 * tile, 2, 96, what="one chunk")
    check_embed(1, 1, 2, 2 * (2 * chunk + 3) - 1, 2, 96, what="two chunks and three")
    check_embed(1, 1, 2, 2 * (2 * chunk + 3) - 1, 2, 6, what="two chunks and three")


@pytest.mark.parametrize("norm,bias", [(False, True), (True, False), (False, False)], ids=["no-norm", "no-bias", "neither"])
def test_embedding_without_a_norm_or_a_projection_bias(norm, bias):
    check_embed(3, 3, 10, 13, 4, 96, (F32, F32), norm, bias)
    check_embed(3, 3, 10, 13, 4, 6, (F32, F32), norm, bias)


EMBED_MIXES = [(F32, F32)] + [m for h in (BF16, F16) for m in ((h, h), (F32, h))]


@pytest.mark.parametrize("mix", EMBED_MIXES, ids=lambda m: "-".join(str(t).split(".")[1] for t in m))
def test_embedding_in_every_accepted_dtype_mix(mix):
    check_embed(3, 3, 10, 13, 4, 192, mix)
    check_embed(3, 3, 10, 13, 4, 6, mix, False, True)


def test_embedding_takes_the_composite_in_float64_and_for_a_gradient_of_the_image(monkeypatch):
    from devis_amd import _swinends
    import devis_amd
    d = on_gpu(embed_case(1, 3, 10, 13, 4, 96)[0])
    monkeypatch.setattr(_swinends, "embed_forward", lambda *a: pytest.fail("the kernel ran"))
    image = d["image"].detach().requires_grad_(True)
    tokens = devis_amd.patch_embed_norm(image, d["proj_weight"], d["proj_bias"], d["norm_weight"], d["norm_bias"])
    assert torch.autograd.grad(tokens, image, d["grad_tokens"])[0].shape == image.shape
    devis_amd.patch_embed_norm(d["image"].double(), *(d[k].double() for k in ("proj_weight", "proj_bias", "norm_weight", "norm_bias")))


def test_each_embedding_gradient_alone_has_the_bits_of_the_full_backward():
    d = on_gpu(embed_case(3, 3, 10, 13, 4, 260)[0])
    full = run_embed(d)
    again = run_embed(d)
    assert all_same_bits(again, full)                                                    # two runs: the same bits
    for i, name in enumerate(EMBED_GRADS):
        alone = run_embed(d, wants=tuple(j == i for j in range(4)))
        assert same_bits(alone[name], full[name]), name
        assert all(alone[other] is None for other in EMBED_GRADS if other != name)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_a_token_has_the_same_bits_alone_in_a_batch_and_for_offset_operands(dtype):
    for C in (96, 6):
        d = on_gpu(embed_case(3, 3, 10, 13, 4, C, (dtype, dtype))[0])
        batch = run_embed(d)
        for b in range(3):
            one = dict(d, image=d["image"][b:b + 1].clone(), grad_tokens=d["grad_tokens"][b:b + 1].clone())
            assert same_bits(run_embed(one)["tokens"], batch["tokens"][b:b + 1]), (C, b)
        for names in (("image",), ("proj_weight", "proj_bias"), ("norm_weight", "norm_bias"), ("grad_tokens",), tuple(d)):
            views = {k: (shifted(v) if k in names else v) for k, v in d.items()}
            assert all_same_bits(run_embed(views), batch), (C, names)


def test_a_16_bit_embedding_is_the_float32_one_rounded_once():
    d = on_gpu(embed_case(3, 3, 10, 13, 4, 192)[0])
    import devis_amd
    args = [d[k] for k in ("image", "proj_weight", "proj_bias", "norm_weight", "norm_bias")]
    with torch.no_grad():
        t32 = devis_amd.patch_embed_norm(*args)
        for half in (BF16, F16):
            assert same_bits(devis_amd.patch_embed_norm(*args, out_dtype=half), t32.to(half))


# ---- layer_norm_to_map -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def map_case(B, H, W, C, mix=(F32, F32, F32)):
    """``mix`` = (x, y, parameters)."""
    xdt, ydt, pdt = mix
    d = {"x": rand(B, H * W, C, seed=11, dtype=xdt), "weight": rand(C, seed=12, dtype=pdt, shift=1.0), "bias": rand(C, seed=13, dtype=pdt),
         "grad_y": rand(B, C, H, W, seed=14, dtype=ydt)}
    want = O.map_forward(d["x"], H, W, d["weight"], d["bias"])
    want.update(O.map_grads(d["x"], H, W, d["weight"], 1e-5, d["grad_y"]))
    return d, want


def run_map(d, H, W, out_dtype=None, wants=(True, True, True)):
    import devis_amd
    leaves = [d[k].detach().requires_grad_(w) for k, w in zip(("x", "weight", "bias"), wants)]
    y = devis_amd.layer_norm_to_map(leaves[0], H, W, leaves[1], leaves[2], out_dtype=out_dtype)
    asked = [t for t in leaves if t.requires_grad]
    grads = iter(torch.autograd.grad(y, asked, d["grad_y"]))
    got = {"y": y.detach()}
    got.update({name: (next(grads) if w else None) for name, w in zip(MAP_GRADS, wants)})
    return got


def check_map(B, H, W, C, mix=(F32, F32, F32)):
    d, want = map_case(B, H, W, C, mix)
    got = run_map(on_gpu(d), H, W, out_dtype=mix[1])
    assert got["y"].dtype == mix[1] and got["y"].is_contiguous() and tuple(got["y"].shape) == (B, C, H, W)
    assert_close(got["y"], want["y"], TOL[mix[1]], "map y %s" % ((B, H, W, C),))
    for name, dt in zip(MAP_GRADS, (mix[0], mix[2], mix[2])):
        assert got[name].dtype == dt
        assert_close(got[name], want[name], TOL[dt], "map %s %s" % (name, (B, H, W, C)))


@pytest.mark.parametrize("C", MAP_CHANNELS)
def test_output_norm_matches_the_oracle_at_every_channel_count(C):
    check_map(3, 5, 7, C)               # a token tile spans batch entries and the last one is partial


def test_output_norm_matches_the_oracle_on_small_and_tile_sized_maps():
    from devis_amd import _swinends
    tile = _swinends.tile(_swinends.TILE_TOKENS)
    for H, W in ((1, 1), (8, 8), (1, tile), (1, tile + 1)):
        check_map(2, H, W, 96)
        check_map(1, H, W, 6)


MAP_MIXES = [(F32, F32, F32)] + [m for h in (BF16, F16) for m in ((h, h, h), (F32, h, F32), (h, h, F32))]


@pytest.mark.parametrize("mix", MAP_MIXES, ids=lambda m: "-".join(str(t).split(".")[1] for t in m))
def test_output_norm_in_every_accepted_dtype_mix(mix):
    check_map(3, 5, 7, 260, mix)
    check_map(3, 5, 7, 6, mix)


def test_a_channels_last_gradient_is_made_dense():
    d = on_gpu(map_case(3, 5, 7, 96)[0])
    dense = run_map(d, 5, 7)
    d["grad_y"] = d["grad_y"].contiguous(memory_format=torch.channels_last)
    assert not d["grad_y"].is_contiguous()
    assert all_same_bits(run_map(d, 5, 7), dense)


@pytest.mark.parametrize("mix", [(F32, F32, F32), (BF16, BF16, F32), (F32, BF16, F32)], ids=["float32", "bfloat16", "mixed"])
def test_output_norm_has_the_bits_of_residual_layer_norm_permuted(mix):
    import devis_amd
    for B, H, W, C in ((3, 5, 7, 96), (3, 5, 7, 6), (2, 5, 7, 1536), (2, 3, 11, 260)):
        d = on_gpu(map_case(B, H, W, C, mix)[0])
        got = run_map(d, H, W, out_dtype=mix[1])
        assert all_same_bits(run_map(d, H, W, out_dtype=mix[1]), got)                     # two runs: the same bits
        x = d["x"].detach().requires_grad_(True)
        _, y = devis_amd.residual_layer_norm(x, None, d["weight"], d["bias"], 1e-5, out_dtype=mix[1])
        grad_tokens = d["grad_y"].permute(0, 2, 3, 1).reshape(B, H * W, C).contiguous()
        grad_x, = torch.autograd.grad(y, x, grad_tokens)
        assert same_bits(got["y"], y.detach().view(B, H, W, C).permute(0, 3, 1, 2).contiguous()), (B, H, W, C)
        assert same_bits(got["grad_x"], grad_x), (B, H, W, C)
        alone = run_map(d, H, W, out_dtype=mix[1], wants=(True, False, False))
        assert same_bits(alone["grad_x"], got["grad_x"]) and alone["grad_weight"] is None
        params = run_map(d, H, W, out_dtype=mix[1], wants=(False, True, True))
        assert same_bits(params["grad_weight"], got["grad_weight"]) and same_bits(params["grad_bias"], got["grad_bias"])
        views = {k: shifted(v) for k, v in d.items()}
        assert all_same_bits(run_map(views, H, W, out_dtype=mix[1]), got), (B, H, W, C)


# ---- stale memory ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF16])
def test_results_over_stale_memory_are_complete_and_stay_inside(monkeypatch, dtype):
    """Outputs, statistics, gradients and the workspaces are handed out holding NaN payloads between guard zones: every element
    is written before it is read, and nothing outside is touched."""
    from devis_amd.functions import swin_ends
    for case in ((3, 3, 10, 13, 4, 96), (2, 3, 3, 5, 4, 6), (1, 1, 2, 2 * 1027 - 1, 2, 260)):
        d = on_gpu(embed_case(*case, (dtype, dtype))[0])
        clean = run_embed(d)
        with monkeypatch.context() as m:
            shim = stale_memory.install(m, [swin_ends])
            got = run_embed(d)
            assert len(shim.buffers) >= 8 and shim.guards_intact()
        assert all(bool(t.isfinite().all()) for t in got.values()) and all_same_bits(got, clean)
    for B, H, W, C in ((3, 5, 7, 96), (1, 1, 1, 6), (2, 5, 7, 260)):
        d = on_gpu(map_case(B, H, W, C, (dtype, dtype, F32))[0])
        clean = run_map(d, H, W)
        with monkeypatch.context() as m:
            shim = stale_memory.install(m, [swin_ends])
            got = run_map(d, H, W)
            assert len(shim.buffers) >= 7 and shim.guards_intact()
        assert all(bool(t.isfinite().all()) for t in got.values()) and all_same_bits(got, clean)


# ---- the backbone ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("others", [False, True], ids=["alone", "with-glue-and-attention"])
def test_patched_backbone_reproduces_the_fixture_on_the_gpu(monkeypatch, others):
    import devis_amd
    import swinends_cases as S
    from devis_amd import _swinends
    case = S.load_fixture()
    calls = []
    for name in ("embed_forward", "embed_backward", "map_forward", "map_backward"):
        monkeypatch.setattr(_swinends, name, lambda *a, _f=getattr(_swinends, name), _n=name: (calls.append(_n), _f(*a))[1])
    undo = []
    if others:
        undo.append((devis_amd.unpatch_window_attention, devis_amd.patch_window_attention(S)))
        undo.append((devis_amd.unpatch_swin_glue, devis_amd.patch_swin_glue(S)))
    undo.append((devis_amd.unpatch_swin_ends, devis_amd.patch_swin_ends(S)))
    try:
        model, image = S.build_backbone(case, torch.float32, DEV)
        got = S.run_backbone(model, image, case)
    finally:
        for f, previous in reversed(undo):
            f(S, previous)
    assert calls.count("embed_forward") == 1 and calls.count("map_forward") == 2 and calls.count("embed_backward") == 1 and \
        calls.count("map_backward") == 2
    for name, want in S.expected(case).items():
        assert_close(got[name], want, 1e-4, "backbone " + name)
