"""CPU tests of the two ends of the Swin backbone (include/swinends.h): the C ABI's argument checks without
a GPU, the torch composites against the float64 oracle, and -- through the test double tests/fake_swinends.py -- the host logic:
which gradients are computed, the patched stand-in backbone against the fixture recorded from the reference, the fallbacks to
the installed forwards, the order of patching with the two other Swin patches, and the no-copy view of the tokens."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

import fake_swinends
import swinends_cases as S
import swinends_oracle as O
from conftest import ROOT

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def close(got, want, tol, what):
    err, ref = float((got.detach().double() - want).abs().max()), float(want.abs().max())
    assert got.shape == want.shape and err <= tol * ref, (what, err, ref)


def rand(*shape, seed=0, dtype=F64):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64).to(dtype)


def embed_inputs(B=2, Cin=3, H=10, W=13, p=4, C=8, norm=True, bias=True):
    L = (-(-H // p)) * (-(-W // p))
    return {"image": rand(B, Cin, H, W, seed=1), "proj_weight": rand(C, Cin, p, p, seed=2) / 4, "proj_bias": rand(C, seed=3) if bias else None,
            "norm_weight": rand(C, seed=4) + 1 if norm else None, "norm_bias": rand(C, seed=5) if norm else None,
            "grad_tokens": rand(B, L, C, seed=6)}


PARAMS = ("proj_weight", "proj_bias", "norm_weight", "norm_bias")


# ---- library -----------------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_swinends_h_declares_and_versions_agree():
    from devis_amd import _binding, _prenorm, _swinends, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "swinends.h")).read()
    declared = set(re.findall(r"\b(swinends_[a-z_0-9]+)\s*\(", header.split("#ifndef SWINENDS_H")[1]))
    assert declared == set(_swinends.EXPORTED_SYMBOLS) and len(declared) == 10
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _swinends.load()
    assert lib.swinends_version() == _swinends.SWINENDS_ABI_VERSION == int(re.search(r"#define SWINENDS_ABI_VERSION (\d+)", header).group(1))
    limits = {name: int(v) for name, v in re.findall(r"#define SWINENDS_MAX_(PATCH|EMBED|CHANNELS) (\d+)", header)}
    assert limits == {"PATCH": _swinends.MAX_PATCH, "EMBED": _swinends.MAX_EMBED, "CHANNELS": _swinends.MAX_CHANNELS}
    assert _swinends.MAX_PATCH >= 192 and _swinends.MAX_EMBED >= 1024 and _swinends.MAX_CHANNELS == _prenorm.MAX_CHANNELS
    assert [_swinends.tile(w) for w in (2, 3, 4)] == [limits["PATCH"], limits["EMBED"], limits["CHANNELS"]]
    tile, chunk = _swinends.tile(_swinends.TILE_TOKENS), _swinends.tile(_swinends.TILE_EMBED_CHUNK)
    assert tile >= 1 and chunk % tile == 0 and lib.swinends_tile(9) == -1
    assert dict(re.findall(r"SWINENDS_(F32|BF16|F16) = (\d)", header)) == {"F32": "0", "BF16": "2", "F16": "3"}
    assert ctypes.sizeof(_swinends.EmbedShape) == 32 and ctypes.sizeof(_swinends.MapShape) == 24
    for struct, cls in (("embed_shape", _swinends.EmbedShape), ("embed_types", _swinends.EmbedTypes), ("map_shape", _swinends.MapShape),
                        ("map_types", _swinends.MapTypes)):
        fields = re.search(r"typedef struct swinends_%s \{(.*?)\}" % struct, header, re.S).group(1)
        assert re.findall(r"\b([A-Za-z]+)\b(?=[,;])", re.sub(r"/\*.*?\*/", "", fields, flags=re.S)) == [n for n, _ in cls._fields_]
    assert os.path.join(build.include_dir(), "swinends.h") in build._headers()
    assert any(s.endswith("swinends.hip") for s in build.sources())
    assert "swinends.h" in open(os.path.join(ROOT, "setup.py")).read() and "swinends.h" in build.include_dir.__doc__
    assert "_swinends" in _binding.__doc__
    source = open(os.path.join(ROOT, "devis_amd", "csrc", "swinends.hip")).read()
    assert re.findall(r'#include "([^"]+)"', source) == ["op_common.h", "swinends.h"] and "atomic" not in source
    # the row code is shared with prenorm.hip, not restated
    shared = open(os.path.join(ROOT, "devis_amd", "csrc", "norm_row.h")).read()
    for unit in (source, open(os.path.join(ROOT, "devis_amd", "csrc", "prenorm.hip")).read()):
        assert "row_sum(" in shared and "row_sum(const" not in unit and "using namespace devis::normrow" in unit


def test_swinends_argument_errors_and_workspace_sizes_without_gpu():
    from devis_amd import _swinends
    lib = _swinends.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.swinends_last_error
    eshape = lambda B=2, Cin=3, H=10, W=13, p=4, C=8: ctypes.byref(_swinends.EmbedShape(B, Cin, H, W, p, C))      # noqa: E731
    etypes = lambda image=0, param=0, y=0: ctypes.byref(_swinends.EmbedTypes(image, param, y))      # noqa: E731
    efwd = lambda t=etypes(), image=p, pw=p, pb=p, nw=p, nb=p, eps=1e-5, s=eshape(), tokens=p, mean=None, rstd=None: \
        lib.swinends_embed_forward(t, image, pw, pb, nw, nb, eps, s, tokens, mean, rstd, None)      # noqa: E731
    ebwd = lambda t=etypes(), image=p, pw=p, pb=p, nw=p, mean=p, rstd=p, gt=p, s=eshape(), wsp=p, gpw=p, gpb=None, gnw=None, gnb=None: \
        lib.swinends_embed_backward(t, image, pw, pb, nw, mean, rstd, gt, s, wsp, gpw, gpb, gnw, gnb, None)      # noqa: E731
    for call in (efwd, ebwd, lambda s=eshape(), **k: lib.swinends_embed_workspace_bytes(s, 1), lambda s=eshape(), **k: lib.swinends_embed_tokens(s)):
        assert call(s=None) == -1 and b"null pointer" in err()
        assert call(s=eshape(C=0)) == -1 and b"positive" in err()
        assert call(s=eshape(C=1025)) == -1 and b"1024" in err()
        assert call(s=eshape(Cin=13)) == -1 and b"192" in err()                # K = 208
        assert call(s=eshape(p=0)) == -1 and call(s=eshape(Cin=0)) == -1 and b"positive" in err()
        assert call(s=eshape(B=-1)) == -1 and b"negative" in err()
        assert call(s=eshape(B=1 << 20, H=1 << 13, W=1 << 13)) == -1 and b"31 bits" in err()
    for call in (efwd, ebwd):
        # float64; a code out of range; 16-bit image beside float32 parameters or tokens; two 16-bit dtypes; 16-bit parameters
        for bad in (dict(image=1, param=1, y=1), dict(image=9), dict(image=2, param=0, y=2), dict(image=2, param=2, y=0),
                    dict(image=2, param=2, y=3), dict(image=0, param=2, y=2)):
            assert call(t=etypes(**bad)) == -1 and b"dtype" in err(), bad
        assert call(t=None) == -1 and b"null pointer" in err()
        for good in (dict(), dict(image=2, param=2, y=2), dict(image=3, param=3, y=3), dict(y=2), dict(y=3)):
            assert call(t=etypes(**good), s=eshape(B=0)) in (0, -1) and b"dtype" not in err(), good
    assert efwd(tokens=None) == -1 and efwd(image=None) == -1 and efwd(pw=None) == -1 and b"null pointer" in err()
    assert efwd(nb=None) == -1 and b"together" in err() and efwd(mean=p) == -1 and b"together" in err()
    assert efwd(nw=None, nb=None, mean=p, rstd=p) == -1 and b"there is none" in err()
    assert efwd(eps=float("nan")) == -1 and b"eps" in err()
    assert ebwd(gpw=None) == -1 and b"no gradient" in err()
    assert ebwd(nw=None) == -1 and b"together" in err() and ebwd(mean=None) == -1 and b"together" in err()
    assert ebwd(nw=None, mean=None, rstd=None, gnw=p) == -1 and b"there is none" in err()
    for name in ("image", "pw", "gt", "wsp"):
        assert ebwd(**{name: None}) == -1 and b"null pointer" in err(), name
    assert ebwd(wsp=ctypes.c_void_p(p.value + 4)) == -1 and b"16-byte" in err()
    for empty in (eshape(B=0), eshape(H=0), eshape(W=0)):                      # nothing to compute: nothing is launched
        assert efwd(s=empty, image=None, pw=None) == 0
    chunk = _swinends.tile(_swinends.TILE_EMBED_CHUNK)
    for B, Cin, H, W, ps, C in ((2, 3, 10, 13, 4, 8), (6, 3, 800, 1333, 4, 192), (1, 1, 2, 2 * chunk, 2, 1024), (1, 1, 2, 2 * chunk + 1, 2, 5)):
        tokens = B * -(-H // ps) * -(-W // ps)
        s = eshape(B, Cin, H, W, ps, C)
        assert lib.swinends_embed_tokens(s) == tokens
        chunks = -(-tokens // chunk)
        for want_weight in (0, 1):
            floats = chunks * (3 + want_weight * Cin * ps * ps) * C
            assert lib.swinends_embed_workspace_bytes(s, want_weight) == -(-(floats * 4) // 256) * 256

    mshape = lambda B=2, H=5, W=7, C=8: ctypes.byref(_swinends.MapShape(B, H, W, C))      # noqa: E731
    mtypes = lambda x=0, y=0, param=0: ctypes.byref(_swinends.MapTypes(x, y, param))      # noqa: E731
    mfwd = lambda t=mtypes(), x=p, w=p, b=p, eps=1e-5, s=mshape(), y=p, mean=None, rstd=None: \
        lib.swinends_map_forward(t, x, w, b, eps, s, y, mean, rstd, None)      # noqa: E731
    mbwd = lambda t=mtypes(), x=p, w=p, mean=p, rstd=p, gy=p, s=mshape(), wsp=p, gx=p, gw=None, gb=None: \
        lib.swinends_map_backward(t, x, w, mean, rstd, gy, s, wsp, gx, gw, gb, None)      # noqa: E731
    for call in (mfwd, mbwd, lambda s=mshape(), **k: lib.swinends_map_workspace_bytes(s)):
        assert call(s=None) == -1 and b"null pointer" in err()
        assert call(s=mshape(C=0)) == -1 and b"positive" in err()
        assert call(s=mshape(C=3073)) == -1 and b"3072" in err()
        assert call(s=mshape(B=-1)) == -1 and b"negative" in err()
        assert call(s=mshape(B=1 << 20, H=1 << 10, W=1 << 10)) == -1 and b"31 bits" in err()
    for call in (mfwd, mbwd):
        for bad in (dict(x=1, y=1, param=1), dict(y=7), dict(x=2, y=0, param=2), dict(x=2, y=3, param=2), dict(x=0, y=0, param=2)):
            assert call(t=mtypes(**bad)) == -1 and b"dtype" in err(), bad
        for good in (dict(), dict(x=2, y=2, param=2), dict(x=3, y=3, param=0), dict(y=2), dict(y=3)):
            assert call(t=mtypes(**good), s=mshape(B=0)) in (0, -1) and b"dtype" not in err(), good
    assert mfwd(y=None) == -1 and mfwd(x=None) == -1 and mfwd(w=None) == -1 and mfwd(b=None) == -1 and b"null pointer" in err()
    assert mfwd(mean=p) == -1 and b"together" in err() and mfwd(eps=float("nan")) == -1 and b"eps" in err()
    assert mfwd(s=mshape(B=0), x=None, w=None, b=None) == 0
    assert mbwd(gx=None) == -1 and b"no gradient" in err()
    for name in ("x", "mean", "rstd", "gy", "w"):
        assert mbwd(**{name: None}) == -1 and b"null pointer" in err(), name
    assert mbwd(gw=p, wsp=None) == -1 and b"workspace" in err()
    assert mbwd(gw=p, wsp=ctypes.c_void_p(p.value + 4)) == -1 and b"16-byte" in err()
    tile = _swinends.tile(_swinends.TILE_TOKENS)
    for B, H, W, C in ((3, 5, 7, 96), (6, 200, 334, 192), (1, 1, tile, 3072), (1, 1, tile + 1, 6)):
        want = -(-(-(-(B * H * W) // tile) * 2 * C * 4) // 256) * 256
        assert lib.swinends_map_workspace_bytes(mshape(B, H, W, C)) == want


# ---- the composites ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("norm,bias", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("size", [(10, 13, 4), (8, 8, 4), (3, 5, 4), (5, 7, 2)])
def test_patch_embed_norm_composite_equals_the_oracle_in_float64(size, norm, bias):
    import devis_amd
    H, W, p = size
    d = embed_inputs(H=H, W=W, p=p, norm=norm, bias=bias)
    leaves = {k: (None if d[k] is None else d[k].clone().requires_grad_(True)) for k in PARAMS}
    tokens = devis_amd.patch_embed_norm(d["image"], *(leaves[k] for k in PARAMS))
    want = O.embed_forward(d["image"], *(d[k] for k in PARAMS))
    want.update(O.embed_grads(d["image"], d["proj_weight"], d["proj_bias"], d["norm_weight"], 1e-5, d["grad_tokens"]))
    close(tokens, want["tokens"], 1e-12, "tokens")
    asked = [k for k in PARAMS if leaves[k] is not None]
    for k, g in zip(asked, torch.autograd.grad(tokens, [leaves[k] for k in asked], d["grad_tokens"])):
        close(g, want["grad_" + k], 1e-11, k)


def test_layer_norm_to_map_composite_equals_the_oracle_in_float64():
    import devis_amd
    B, H, W, C = 3, 5, 7, 6
    x, w, b, gy = rand(B, H * W, C, seed=1).requires_grad_(True), (rand(C, seed=2) + 1).requires_grad_(True), rand(C, seed=3).requires_grad_(True), rand(B, C, H, W, seed=4)
    y = devis_amd.layer_norm_to_map(x, H, W, w, b)
    assert y.is_contiguous() and tuple(y.shape) == (B, C, H, W)
    want = O.map_forward(x.detach(), H, W, w.detach(), b.detach())
    want.update(O.map_grads(x.detach(), H, W, w.detach(), 1e-5, gy))
    close(y, want["y"], 1e-12, "y")
    for name, g in zip(("grad_x", "grad_weight", "grad_bias"), torch.autograd.grad(y, [x, w, b], gy)):
        close(g, want[name], 1e-11, name)
    with pytest.raises(RuntimeError, match="H \\* W"):
        devis_amd.layer_norm_to_map(x, 5, 6, w, b)
    with pytest.raises(RuntimeError, match="proj_weight"):
        devis_amd.patch_embed_norm(rand(1, 3, 8, 8), rand(4, 2, 4, 4), None, None, None)


# ---- through the test double -------------------------------------------------------------------------------------------------

# Through the test double the statistics are saved in float32, as the contract has them (2 ** -24 relative each), so a gradient
# computed from them is held to 1e-6 of its largest value, and the fixture to swinglue's 1e-5.
STATS_TOL = 1e-6


def test_backward_computes_only_the_gradients_autograd_asks_for(monkeypatch):
    import devis_amd
    calls = fake_swinends.install(monkeypatch)
    d = embed_inputs()
    want = O.embed_grads(d["image"], d["proj_weight"], d["proj_bias"], d["norm_weight"], 1e-5, d["grad_tokens"])
    for wants in ((True, True, True, True), (True, False, False, False), (False, False, True, True), (False, True, False, False)):
        del calls[:]
        leaves = [d[k].clone().requires_grad_(w) for k, w in zip(PARAMS, wants)]
        tokens = devis_amd.patch_embed_norm(d["image"], *leaves)
        asked = [t for t in leaves if t.requires_grad]
        grads = iter(torch.autograd.grad(tokens, asked, d["grad_tokens"]))
        assert calls == [("embed_forward", True, True, True), ("embed_backward",) + wants]
        for k, w in zip(PARAMS, wants):
            if w:
                close(next(grads), want["grad_" + k], STATS_TOL, k)
    # a frozen patch embedding launches no backward and keeps no statistics; neither does no_grad
    del calls[:]
    tokens = devis_amd.patch_embed_norm(d["image"], *(d[k] for k in PARAMS))
    assert not tokens.requires_grad and calls == [("embed_forward", True, True, False)]
    # without a norm there are no statistics and two gradients
    del calls[:]
    pw, pb = d["proj_weight"].clone().requires_grad_(True), d["proj_bias"].clone().requires_grad_(True)
    torch.autograd.grad(devis_amd.patch_embed_norm(d["image"], pw, pb, None, None), [pw, pb], d["grad_tokens"])
    assert calls == [("embed_forward", False, True, False), ("embed_backward", True, True, False, False)]
    # an image that requires a gradient takes the composite
    del calls[:]
    image = d["image"].clone().requires_grad_(True)
    tokens = devis_amd.patch_embed_norm(image, *(d[k] for k in PARAMS))
    assert calls == [] and torch.autograd.grad(tokens, image, d["grad_tokens"])[0].shape == image.shape
    # the output norm
    B, H, W, C = 2, 3, 4, 6
    x, w, b, gy = rand(B, H * W, C, seed=1), rand(C, seed=2) + 1, rand(C, seed=3), rand(B, C, H, W, seed=4)
    want = O.map_grads(x, H, W, w, 1e-5, gy)
    for wants in ((True, True, True), (True, False, False), (False, True, True)):
        del calls[:]
        leaves = [t.clone().requires_grad_(on) for t, on in zip((x, w, b), wants)]
        y = devis_amd.layer_norm_to_map(*leaves[:1], H, W, *leaves[1:])
        grads = iter(torch.autograd.grad(y, [t for t in leaves if t.requires_grad], gy.contiguous(memory_format=torch.channels_last)))
        assert calls == [("map_forward", H, W, C), ("map_backward",) + wants]
        for name, on in zip(("grad_x", "grad_weight", "grad_bias"), wants):
            if on:
                close(next(grads), want[name], STATS_TOL, name)
    del calls[:]
    with torch.no_grad():
        devis_amd.layer_norm_to_map(x.requires_grad_(True), H, W, w, b)
    assert calls == [("map_forward", H, W, C)]


def check_fixture(got, case, tol, what):
    want = S.expected(case)
    assert sorted(got) == sorted(want), what
    for key in sorted(got):
        close(got[key], want[key], tol, "%s %s" % (what, key))


def test_patched_backbone_issues_the_expected_calls_and_reproduces_the_fixture(monkeypatch):
    import devis_amd
    calls = fake_swinends.install(monkeypatch)
    case = S.load_fixture()
    model, image = S.build_backbone(case)
    previous = devis_amd.patch_swin_ends(S)
    try:
        got = S.run_backbone(model, image, case)
        check_fixture(got, case, 1e-5, "patched backbone")
        assert [c[0] for c in calls] == ["embed_forward", "map_forward", "map_forward", "map_backward", "map_backward", "embed_backward"]
        assert calls[-1] == ("embed_backward", True, True, True, True) and calls[3] == ("map_backward", True, True, True)
        # a frozen patch embedding (frozen_stages >= 0): no backward of it is launched
        del calls[:]
        for param in model.patch_embed.parameters():
            param.requires_grad = False
        outs = model(image)
        torch.autograd.grad([outs["0"].sum(), outs["1"].sum()], [p for p in model.parameters() if p.requires_grad])
        assert [c[0] for c in calls].count("embed_backward") == 0 and calls[0] == ("embed_forward", True, True, False)
        # the tokens come back without a copy: the NCHW view flattens into the dense token tensor
        x = model.patch_embed(image)
        assert tuple(x.shape) == (2, 8, 3, 4) and tuple(x.stride()) == (96, 1, 32, 8)
        tokens = x.flatten(2).transpose(1, 2)
        assert tokens.data_ptr() == x.data_ptr() and tokens.is_contiguous() and tuple(tokens.shape) == (2, 12, 8)
        # without a patch norm the tokens are the projection
        plain, _ = S.build_backbone(None, patch_norm=False)
        want = getattr(S.PatchEmbed, "_devis_amd_ends_previous_forward")(plain.patch_embed, image)
        del calls[:]
        close(plain.patch_embed(image), want.detach(), 1e-12, "patch_norm=False")
        assert calls[0][:2] == ("embed_forward", False)
    finally:
        devis_amd.unpatch_swin_ends(S, previous)


def test_patched_backbone_on_the_cpu_runs_the_installed_forwards_and_reproduces_the_fixture(monkeypatch):
    import devis_amd
    from devis_amd import _swinends
    for name in ("embed_forward", "map_forward"):
        monkeypatch.setattr(_swinends, name, lambda *a: pytest.fail("a kernel was asked for on the CPU"))
    case = S.load_fixture()
    model, image = S.build_backbone(case)
    previous = devis_amd.patch_swin_ends(S)
    try:
        check_fixture(S.run_backbone(model, image, case), case, 1e-9, "cpu")
    finally:
        devis_amd.unpatch_swin_ends(S, previous)
    assert "_devis_amd_ends_previous_forward" not in S.PatchEmbed.__dict__


def test_each_fallback_condition_reaches_the_installed_forward(monkeypatch):
    import devis_amd
    from devis_amd.modules import swin_ends as module
    calls = fake_swinends.install(monkeypatch)
    seen = []
    stock_embed, stock_backbone = S.PatchEmbed.forward, S.SwinTransformer.forward
    monkeypatch.setattr(S.PatchEmbed, "forward", lambda self, x: (seen.append("embed"), stock_embed(self, x))[1])
    monkeypatch.setattr(S.SwinTransformer, "forward", lambda self, x: (seen.append("backbone"), stock_backbone(self, x))[1])
    previous = devis_amd.patch_swin_ends(S)
    try:
        model, image = S.build_backbone(None)

        def run(expect_embed, expect_backbone, what, m=model, x=image):
            del calls[:], seen[:]
            with torch.no_grad():
                m(x)
            assert ("embed" in seen, "backbone" in seen) == (expect_embed, expect_backbone), what
            assert any(c[0] == "embed_forward" for c in calls) == (not expect_embed), what
            assert any(c[0] == "map_forward" for c in calls) == (not expect_backbone), what

        run(False, False, "fused")
        with monkeypatch.context() as m:                    # while compiling
            m.setattr(torch.compiler, "is_compiling", lambda: True)
            run(True, True, "compiling")
        with monkeypatch.context() as m:                    # CPU tensors
            m.setattr(module, "_on_gpu", lambda t: False)
            run(True, True, "cpu")
        with monkeypatch.context() as m:                    # float64
            from devis_amd.functions import swin_ends
            m.setattr(swin_ends, "DTYPES", swin_ends.DTYPES[:3])
            run(True, True, "float64")
        other, _ = S.build_backbone(None, norm_layer=lambda C: nn.LayerNorm(C, elementwise_affine=False))
        run(True, True, "norms that are not affine", other)
        other, _ = S.build_backbone(None)
        other.norm1 = nn.Identity()
        run(False, True, "an output norm that is no LayerNorm", other)
        for change in (dict(padding=(1, 1)), dict(dilation=(2, 2)), dict(stride=(2, 2)), dict(groups=3), dict(padding="same")):
            other, _ = S.build_backbone(None)
            assert module._plain_projection(other.patch_embed.proj)
            for key, value in change.items():
                monkeypatch.setattr(other.patch_embed.proj, key, value)
            assert not module._plain_projection(other.patch_embed.proj), change
            if "groups" in change or change.get("padding") == "same":
                continue                                     # (the stock convolution itself refuses these)
            del calls[:], seen[:]
            with torch.no_grad():
                other.patch_embed(image)
            assert seen == ["embed"] and not calls, change
        other, _ = S.build_backbone(None)
        other.patch_embed.proj = nn.Sequential(other.patch_embed.proj)
        run(True, False, "a projection that is no Conv2d", other)
        with monkeypatch.context() as m:                    # above the limits
            from devis_amd import _swinends
            m.setattr(_swinends, "MAX_PATCH", 47)
            run(True, False, "K above the limit")
        with monkeypatch.context() as m:
            m.setattr(_swinends, "MAX_EMBED", 7)
            run(True, False, "C above the embedding's limit")
        with monkeypatch.context() as m:
            m.setattr(_swinends, "MAX_CHANNELS", 15)
            run(False, True, "C above the norm's limit")
    finally:
        devis_amd.unpatch_swin_ends(S, previous)


def test_patching_and_unpatching_with_the_two_other_swin_patches_in_any_order_restores_the_forwards():
    import itertools

    import devis_amd
    classes = (S.PatchEmbed, S.SwinTransformer, S.SwinTransformerBlock, S.BasicLayer, S.PatchMerging)
    stock = [cls.forward for cls in classes]
    patches = {"ends": (devis_amd.patch_swin_ends, devis_amd.unpatch_swin_ends), "glue": (devis_amd.patch_swin_glue, devis_amd.unpatch_swin_glue),
               "attention": (devis_amd.patch_window_attention, devis_amd.unpatch_window_attention)}
    from devis_amd.modules import swin_ends as module
    for order in itertools.permutations(patches):
        undo = [(patches[name][1], patches[name][0](S)) for name in order]
        assert S.PatchEmbed.forward is module.embed_forward and S.SwinTransformer.forward is module.backbone_forward
        for unpatch, previous in reversed(undo):
            unpatch(S, previous)
        assert [cls.forward for cls in classes] == stock, order
        assert not any("_devis_amd_ends_previous_forward" in cls.__dict__ for cls in classes)
    # patched twice: the recorded forward stays the stock one
    first = devis_amd.patch_swin_ends(S)
    second = devis_amd.patch_swin_ends(S)
    assert second == first and getattr(S.PatchEmbed, "_devis_amd_ends_previous_forward") is stock[0]
    devis_amd.unpatch_swin_ends(S, second)
    assert [cls.forward for cls in classes] == stock


def test_the_documents_describe_the_operators():
    for name, words in (("DESIGN.md", ("## 24.", "swinends.h", "patch_embed_norm", "layer_norm_to_map")),
                        ("INTEGRATION.md", ("Backbone: Swin patch embedding and output norms", "patch_swin_ends")),
                        ("README.md", ("patch_swin_ends", "swinends_bench"))):
        text = open(os.path.join(ROOT, name)).read()
        for word in words:
            assert word in text, (name, word)
    assert os.path.exists(os.path.join(ROOT, "profiles", "swinends_resource_usage.txt"))
