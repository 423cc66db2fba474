"""CPU tests of the mask loss: the oracle against the reference fixtures and against F.interpolate, the C ABI of
include/maskloss.h (exports, version, argument errors, workspace arithmetic -- no compute calls), the host code (shape checks,
errors, no backward call without a gradient to compute), the drop-in loss_masks and its patch functions, and the fake-tensor
paths.  The kernels themselves are tests/test_maskloss_gpu.py."""
import ctypes
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

import maskloss_oracle
from conftest import ROOT, golden, golden_names

FIXTURES = golden_names("maskloss_")
F64 = torch.float64


def load_fixture(name):
    """The arrays of one fixture as tensors; ``alpha`` and ``num_boxes`` as Python floats."""
    d = {k: torch.from_numpy(v) for k, v in golden(name).items()}
    d["alpha"], d["num_boxes"] = float(d["alpha"]), float(d["num_boxes"])
    return d


def stock_losses(src, target, num_boxes, alpha=0.25, gamma=2.0):
    """The stock formulation, written out with torch's own operators (the test suite's restatement of what the criterion
    computes): interpolate, binary_cross_entropy_with_logits, the focal modulation, the dice ratio.  src [N, h, w]."""
    x = F.interpolate(src[:, None], size=target.shape[-2:], mode="bilinear", align_corners=False)[:, 0].flatten(1)
    t = target.to(x).flatten(1)
    p = x.sigmoid()
    loss = F.binary_cross_entropy_with_logits(x, t, reduction="none") * (1 - (p * t + (1 - p) * (1 - t))) ** gamma
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    dice = 1 - (2 * (p * t).sum(1) + 1) / (p.sum(-1) + t.sum(-1) + 1)
    return loss.mean(1).sum() / num_boxes, dice.sum() / num_boxes


# ---- oracle ----------------------------------------------------------------------------------------------------------

def test_fixtures_cover_the_cases():
    assert FIXTURES == ["maskloss_down", "maskloss_noalpha", "maskloss_up", "maskloss_video"]
    shapes = {}
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 32 << 10
        d = load_fixture(name)
        assert d["target"].dtype == torch.bool and d["src"].dtype == F64
        shapes[name] = (tuple(d["src"].shape), tuple(d["target"].shape))
    assert shapes["maskloss_up"] == ((3, 7, 9), (3, 27, 35))
    assert shapes["maskloss_video"] == ((4, 12, 20), (4, 45, 80))
    assert shapes["maskloss_down"] == ((2, 26, 22), (2, 13, 11))
    video = load_fixture("maskloss_video")["target"]
    assert not bool(video[1].any()) and bool(video[2].all())
    assert load_fixture("maskloss_noalpha")["alpha"] == -1.0 and load_fixture("maskloss_up")["alpha"] == 0.25


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_equals_the_reference_losses_and_gradient(name):
    d = load_fixture(name)
    # (the reference ran F.interpolate in float64, whose taps are float64 too)
    lm, ld, grad = maskloss_oracle.mask_losses(d["src"], d["target"], d["num_boxes"], d["alpha"], arith=F64, with_grad=True)
    for got, want in ((lm, d["loss_mask"]), (ld, d["loss_dice"]), (grad, d["grad_src"])):
        assert got.dtype == F64 and float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    # and the suite's restatement of the stock formulation is the reference's
    sm, sd = stock_losses(d["src"], d["target"], d["num_boxes"], d["alpha"])
    assert abs(float(sm - d["loss_mask"])) <= 1e-12 and abs(float(sd - d["loss_dice"])) <= 1e-12


@pytest.mark.parametrize("gamma", [0.0, 1.0, 2.0, 3.0])
def test_oracle_gradient_is_the_gradient_of_the_stock_formulation(gamma):
    g = torch.Generator().manual_seed(5)
    src = (2 * torch.randn(3, 6, 5, generator=g, dtype=F64)).requires_grad_(True)
    target = torch.rand(3, 17, 13, generator=g, dtype=F64)         # soft targets too
    gf, gd = torch.randn(3, generator=g, dtype=F64), torch.randn(3, generator=g, dtype=F64)
    focal, dice, grad = maskloss_oracle.mask_loss_terms(src.detach(), target, 0.3, gamma, arith=F64, grads=(gf, gd))
    x = F.interpolate(src[:, None], size=(17, 13), mode="bilinear", align_corners=False)[:, 0]
    p = x.sigmoid()
    fl = F.binary_cross_entropy_with_logits(x, target, reduction="none") * (1 - (p * target + (1 - p) * (1 - target))) ** gamma
    fl = ((0.3 * target + 0.7 * (1 - target)) * fl).flatten(1).mean(1)
    dc = 1 - (2 * (p * target).flatten(1).sum(1) + 1) / (p.flatten(1).sum(1) + target.flatten(1).sum(1) + 1)
    want, = torch.autograd.grad((fl * gf).sum() + (dc * gd).sum(), src)
    assert float((focal - fl).abs().max()) <= 1e-12 and float((dice - dc).abs().max()) <= 1e-12
    assert float((grad - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("pair", [(7, 27), (14, 46), (12, 45), (26, 13), (5, 5), (1, 7)])
def test_oracle_upsampling_equals_f_interpolate(pair):
    a, b = pair
    g = torch.Generator().manual_seed(a * 100 + b)
    for arith, tol in ((torch.float32, 1e-6), (F64, 1e-14)):
        src = torch.randn(2, a, a + 2, generator=g, dtype=arith)
        want = F.interpolate(src[:, None], size=(b, b + 3), mode="bilinear", align_corners=False)[:, 0].double()
        got = maskloss_oracle.resample(src, (b, b + 3), arith)
        assert float((got - want).abs().max()) <= tol * float(want.abs().max())
    i0, i1, l0, l1 = maskloss_oracle.taps(a, b)
    assert int(i0.min()) >= 0 and int(i1.max()) <= a - 1 and bool(((i1 - i0) >= 0).all()) and bool(((i1 - i0) <= 1).all())
    if a == b:
        assert torch.equal(i0, torch.arange(a)) and float(l1.abs().max()) == 0.0        # the identity


@pytest.mark.parametrize("pair", [(14, 46), (12, 45)])
@pytest.mark.parametrize("rule", ["align_corners", "integer"])
def test_a_wrong_tap_rule_is_far_outside_the_tolerance(pair, rule):
    """tests/test_maskloss_gpu.py::test_tap_rule compares at 1e-4 on these sizes: a kernel with another rule must miss it by
    more than a factor of ten, or that test would not tell the rules apart."""
    a, b = pair
    g = torch.Generator().manual_seed(7)
    src = (2.5 * torch.randn(3, a, a, generator=g, dtype=F64)).float()
    target = torch.rand(3, b, b, generator=g) > 0.5
    ones = torch.ones(3, dtype=F64)
    right = maskloss_oracle.mask_loss_terms(src, target, grads=(ones, ones))
    wrong = maskloss_oracle.mask_loss_terms(src, target, rule=rule, grads=(ones, ones))
    for r, w in zip(right, wrong):
        assert float((r - w).abs().max()) > 10 * 1e-4 * float(r.abs().max())


# ---- library ---------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_maskloss_h_declares_and_versions_agree():
    from devis_amd import _maskloss, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "maskloss.h")).read()
    declared = set(re.findall(r"\b(maskloss_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_maskloss.EXPORTED_SYMBOLS) and len(declared) == 6
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _maskloss.load()
    assert lib.maskloss_version() == _maskloss.MASKLOSS_ABI_VERSION == int(re.search(r"#define MASKLOSS_ABI_VERSION (\d+)", header).group(1))
    tiles = tuple(int(re.search(r"#define MASKLOSS_TILE_%s (\d+)" % n, header).group(1))
                  for n in ("FWD_PIXELS", "FWD_SRC", "BWD_ROWS", "BWD_COLS", "BWD_CHUNK"))
    assert tiles == (_maskloss.TILE_FWD_PIXELS, _maskloss.TILE_FWD_SRC, _maskloss.TILE_BWD_ROWS, _maskloss.TILE_BWD_COLS,
                     _maskloss.TILE_BWD_CHUNK)
    assert all(_maskloss.tile(t) > 0 for t in tiles) and lib.maskloss_tile(9) == -1
    assert _maskloss.tile(_maskloss.TILE_FWD_PIXELS) % 16 == 0
    assert dict(re.findall(r"MASKLOSS_(F32|F64|BF16|F16) = (\d)", header)) == {"F32": "0", "F64": "1", "BF16": "2", "F16": "3"}
    kinds = dict(re.findall(r"MASKLOSS_TARGET_(U8|SAME|F32) = (\d)", header))
    assert kinds == {"U8": str(_maskloss.TARGET_U8), "SAME": str(_maskloss.TARGET_SAME), "F32": str(_maskloss.TARGET_F32)}
    assert "max(scale * (d + 0.5f) - 0.5f, 0)" in header               # the tap rule is stated
    assert os.path.join(build.include_dir(), "maskloss.h") in build._headers()
    assert any(s.endswith("maskloss.hip") for s in build.sources())
    assert "maskloss.h" in open(os.path.join(ROOT, "setup.py")).read()


def _shape(**kw):
    from devis_amd import _maskloss
    d = dict(N=6, h=12, w=20, H=45, W=80)
    d.update(kw)
    return _maskloss.Shape(**d)


def test_maskloss_argument_errors_without_gpu():
    from devis_amd import _maskloss
    lib = _maskloss.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = ctypes.byref(_shape())
    err = lib.maskloss_last_error

    def fwd(dtype=0, kind=0, src=p, target=p, shape=ok, alpha=0.25, gamma=2.0, ws=p, focal=p, dice=p, sums=p):
        return lib.maskloss_forward(dtype, kind, src, target, shape, alpha, gamma, ws, focal, dice, sums, None)

    def bwd(dtype=0, kind=0, src=p, target=p, sums=p, gf=p, gd=p, shape=ok, alpha=0.25, gamma=2.0, gs=p):
        return lib.maskloss_backward(dtype, kind, src, target, sums, gf, gd, shape, alpha, gamma, gs, None)

    for call in (fwd, bwd):
        assert call(dtype=9) == -1 and b"dtype" in err()
        assert call(dtype=-1) == -1 and b"dtype" in err()
        assert call(kind=3) == -1 and b"target kind" in err()
        assert call(kind=-1) == -1 and b"target kind" in err()
        assert call(shape=None) == -1 and b"null pointer" in err()
        for bad in (dict(h=0), dict(H=0), dict(h=-3), dict(H=-1), dict(w=0), dict(W=0), dict(N=-1)):
            assert call(shape=ctypes.byref(_shape(**bad))) == -1 and b"positive" in err(), bad
        assert call(shape=ctypes.byref(_shape(H=65536, W=65536))) == -1 and b"31 bits" in err()
        assert call(shape=ctypes.byref(_shape(h=65536, w=65536))) == -1 and b"31 bits" in err()
        for gamma in (0.5, 0.999, 1e-3, -1.0, float("nan"), float("inf")):
            assert call(gamma=gamma) == -1 and b"gamma" in err(), gamma
        assert call(alpha=float("nan")) == -1 and b"alpha" in err()
        for name in ("src", "target", "sums"):
            assert call(**{name: None}) == -1 and b"null pointer" in err(), name
    for name in ("focal", "dice"):
        assert fwd(**{name: None}) == -1 and b"null pointer" in err(), name
    for name in ("gf", "gd", "gs"):
        assert bwd(**{name: None}) == -1 and b"null pointer" in err(), name
    assert fwd(ws=None, shape=ctypes.byref(_shape(H=100, W=100))) == -1 and b"workspace" in err()      # three tiles
    # no instance: nothing is launched, nothing is dereferenced
    empty = ctypes.byref(_shape(N=0))
    assert fwd(src=None, target=None, ws=None, focal=None, dice=None, sums=None, shape=empty) == 0
    assert bwd(src=None, target=None, sums=None, gf=None, gd=None, gs=None, shape=empty) == 0


def test_workspace_arithmetic():
    from devis_amd import _maskloss
    lib = _maskloss.load()
    tile = _maskloss.tile(_maskloss.TILE_FWD_PIXELS)
    up = lambda n: (n + 255) // 256 * 256      # noqa: E731

    def want(acc, N, H, W):
        tiles = -(-(H * W) // tile)
        return up(N * tiles * 4 * acc) if tiles > 1 else 0

    for dtype, acc in ((0, 4), (1, 8), (2, 4), (3, 4)):
        assert lib.maskloss_workspace_bytes(dtype, ctypes.byref(_shape(H=100, W=100))) == want(acc, 6, 100, 100) > 0
        assert lib.maskloss_workspace_bytes(dtype, ctypes.byref(_shape(N=120, H=800, W=1333))) == want(acc, 120, 800, 1333)
        assert lib.maskloss_workspace_bytes(dtype, ctypes.byref(_shape(H=tile // 64, W=64))) == 0       # one tile
        assert lib.maskloss_workspace_bytes(dtype, ctypes.byref(_shape(H=1, W=tile + 1))) == want(acc, 6, 1, tile + 1) > 0
    assert lib.maskloss_workspace_bytes(0, ctypes.byref(_shape(N=0, H=100, W=100))) == 0
    assert lib.maskloss_workspace_bytes(7, ctypes.byref(_shape())) == -1 and lib.maskloss_workspace_bytes(0, None) == -1
    with pytest.raises(RuntimeError, match="positive"):
        _maskloss.workspace_bytes(0, _shape(w=0))


# ---- host ------------------------------------------------------------------------------------------------------------

def test_operator_raises_on_cpu_tensors_and_on_bad_arguments_before_any_launch(monkeypatch):
    import devis_amd
    from devis_amd import _maskloss
    from devis_amd.functions import mask_losses as L

    def no_launch(*a, **k):
        raise AssertionError("a kernel call was made")

    monkeypatch.setattr(_maskloss, "forward", no_launch)
    monkeypatch.setattr(_maskloss, "backward", no_launch)
    src, target = torch.zeros(3, 6, 10), torch.zeros(3, 24, 40, dtype=torch.bool)
    for fn in (devis_amd.mask_loss_terms, lambda s, t, **k: devis_amd.mask_losses(s, t, 3.0, **k)):
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            fn(src, target)
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            fn(src[:, None], target)
        with pytest.raises(RuntimeError, match="4 instances, src_masks 3"):
            fn(src, torch.zeros(4, 24, 40, dtype=torch.bool))
        with pytest.raises(RuntimeError, match="\\[N, h, w\\] or \\[N, 1, h, w\\]"):
            fn(torch.zeros(3, 2, 6, 10), target)
        for gamma in (0.5, -1.0, float("nan")):
            with pytest.raises(ValueError, match="gamma"):
                fn(src, target, gamma=gamma)
        with pytest.raises(RuntimeError, match="no gradient"):
            fn(src, torch.zeros(3, 24, 40, requires_grad=True))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        L._backward(torch.zeros(3), torch.zeros(3), src, target, torch.zeros(3, 3), 0.25, 2.0)
    assert devis_amd.mask_losses is devis_amd.ops.mask_losses and devis_amd.mask_loss_terms is devis_amd.ops.mask_loss_terms
    for name in ("mask_loss_terms", "mask_losses", "patch_mask_losses", "unpatch_mask_losses"):
        assert name in devis_amd.__all__ and hasattr(devis_amd, name)

    meta = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="meta")      # noqa: E731
    h = torch.bfloat16
    assert L.check_shapes(meta(3, 6, 10), meta(3, 24, 40, dtype=torch.bool)) == (3, 6, 10, 24, 40, _maskloss.TARGET_U8)
    assert L.check_shapes(meta(3, 6, 10), meta(3, 24, 40, dtype=torch.uint8))[-1] == _maskloss.TARGET_U8
    assert L.check_shapes(meta(3, 6, 10), meta(3, 24, 40))[-1] == _maskloss.TARGET_SAME
    assert L.check_shapes(meta(3, 6, 10, dtype=h), meta(3, 24, 40, dtype=h))[-1] == _maskloss.TARGET_SAME
    assert L.check_shapes(meta(3, 6, 10, dtype=h), meta(3, 24, 40))[-1] == _maskloss.TARGET_F32
    assert L.check_shapes(meta(0, 6, 10), meta(0, 3, 4))[0] == 0
    bad = [
        ("src_masks must be", lambda: L.check_shapes(meta(6, 10), meta(3, 24, 40))),
        ("target_masks must be \\[N, H, W\\]", lambda: L.check_shapes(meta(3, 6, 10), meta(3, 1, 24, 40))),
        ("unsupported dtype", lambda: L.check_shapes(meta(3, 6, 10, dtype=torch.int32), meta(3, 24, 40))),
        ("target_masks must be bool", lambda: L.check_shapes(meta(3, 6, 10), meta(3, 24, 40, dtype=torch.int64))),
        ("target_masks must be bool", lambda: L.check_shapes(meta(3, 6, 10), meta(3, 24, 40, dtype=torch.float64))),
        ("would be empty", lambda: L.check_shapes(meta(3, 0, 10), meta(3, 24, 40))),
        ("would be empty", lambda: L.check_shapes(meta(3, 6, 10), meta(3, 24, 0))),
    ]
    for match, call in bad:
        with pytest.raises(RuntimeError, match=match):
            call()
    assert L.check_gamma(2) == 2.0 and L.check_gamma(0) == 0.0 and L.check_gamma(1) == 1.0 and L.check_gamma(3.5) == 3.5


def test_no_backward_call_when_src_needs_no_gradient():
    from devis_amd import ops
    from devis_amd.functions import mask_losses as L
    seen = []
    src, target, sums = torch.zeros(3, 6, 10), torch.zeros(3, 24, 40, dtype=torch.bool), torch.zeros(3, 3)
    gf, gd = torch.ones(3), torch.ones(3)

    def fake_host_backward(grad_focal, grad_dice, src, target, sums, alpha, gamma):
        seen.append(("host", alpha, gamma))
        return torch.zeros_like(src)

    def fake_op_backward(grad_focal, grad_dice, src, target, sums, alpha, gamma):
        seen.append(("op", alpha, gamma))
        return torch.zeros_like(src)

    # the one formula, run the way the eager Function runs it and the way the op's register_autograd does
    assert L.MaskLossTermsFunction.setup_context is L.setup_context is ops.mask_loss_terms_op._setup_context_fn
    assert ops.mask_loss_terms_op._backward_fn.func is L.backward
    for needs in ((False, False, False, False), (True, False, False, False)):
        ctx = types.SimpleNamespace(saved_tensors=(src, target, sums), needs_input_grad=needs, alpha=0.25, gamma=2.0)
        before = len(seen)
        for run, who in ((fake_host_backward, "host"), (fake_op_backward, "op")):
            res = L.backward(run, ctx, gf, gd, None)
            assert len(res) == 4 and res[1:] == (None, None, None)
            if needs[0]:
                assert seen[-1] == (who, 0.25, 2.0) and tuple(res[0].shape) == (3, 6, 10)
            else:
                assert res[0] is None
        assert len(seen) == before + (2 if needs[0] else 0)


# ---- the drop-in loss_masks and its patch ----------------------------------------------------------------------------------

class StandInCriterion:
    """The index helpers a criterion hands to loss_masks (the suite's own: concatenate per-image indices)."""

    @staticmethod
    def _cat(indices, pick, masked=False):
        batch = torch.cat([torch.full_like(e[pick], i)[e[2]] if masked else torch.full_like(e[pick], i) for i, e in enumerate(indices)])
        return batch, torch.cat([e[pick][e[2]] if masked else e[pick] for e in indices])

    def _get_tgt_permutation_idx(self, indices, from_devis=False):
        assert from_devis == (len(indices[0]) == 3)
        return self._cat(indices, 1)

    def _get_tgt_permutation_masked_idx(self, indices):
        return self._cat(indices, 1, masked=True)

    def loss_masks(self, outputs, targets, indices, num_boxes):
        return "theirs"


def stand_in_case(form, device="cpu", dtype=torch.float32, seed=0):
    """(outputs, targets, indices, the [N, h, w] logits in target order, the [N, H, W] bool targets) for an image matching
    ("image"), a DeVIS matching whose first mask selects something ("devis") and a DeVIS matching of one clip whose mask
    selects nothing ("devis_empty": no instance is left)."""
    g = torch.Generator().manual_seed(seed)
    masks = [torch.rand(3, 20, 28, generator=g) > 0.5, torch.rand(2, 24, 22, generator=g) > 0.5]      # two sizes: padding
    padded = torch.zeros(2, 3, 24, 28, dtype=torch.bool)
    padded[0, :, :20, :28], padded[1, :2, :24, :22] = masks[0], masks[1]
    tgt = [torch.tensor([2, 0]), torch.tensor([1, 0])]
    srcq = [torch.tensor([4, 1]), torch.tensor([0, 3])]
    chosen = [(0, 2), (0, 0), (1, 1), (1, 0)]
    if form == "image":
        indices = [(srcq[0], tgt[0]), (srcq[1], tgt[1])]
    elif form == "devis":
        indices = [(srcq[0], tgt[0], torch.tensor([True, False])), (srcq[1], tgt[1], torch.tensor([True, True]))]
    else:
        masks, chosen = masks[:1], []
        indices = [(srcq[0], tgt[0], torch.tensor([False, False]))]
    targets = [{"masks": m.to(device)} for m in masks]
    want_t = torch.stack([padded[b, i] for b, i in chosen]) if chosen else torch.zeros(0, 20, 28, dtype=torch.bool)
    logits = (2 * torch.randn(len(chosen) or 2, 6, 7, generator=g)).to(dtype)
    pred = logits[:, None] if form == "image" else logits
    want_s = logits if chosen else logits[:0]
    indices = [tuple(e.to(device) for e in entry) for entry in indices]
    return {"pred_masks": pred.to(device)}, targets, indices, want_s, want_t


@pytest.mark.parametrize("form", ["image", "devis", "devis_empty"])
def test_loss_masks_hands_the_operator_small_logits_and_bool_targets(form, monkeypatch):
    from devis_amd import argument_builders, ops
    outputs, targets, indices, want_s, want_t = stand_in_case(form)
    seen = {}

    def fake(src_masks, target_masks, num_boxes, alpha=0.25, gamma=2.0):
        seen.update(src=src_masks, target=target_masks, num_boxes=num_boxes, alpha=alpha, gamma=gamma)
        return {"loss_mask": 1, "loss_dice": 2}

    monkeypatch.setattr(ops, "mask_losses", fake)
    assert argument_builders.loss_masks(StandInCriterion(), outputs, targets, indices, 3.5) == {"loss_mask": 1, "loss_dice": 2}
    assert seen["target"].dtype == torch.bool and torch.equal(seen["target"], want_t)
    assert torch.equal(seen["src"].reshape(want_s.shape), want_s) and seen["num_boxes"] == 3.5
    assert (seen["alpha"], seen["gamma"]) == (0.25, 2.0)
    if form == "devis_empty":
        return
    padded = argument_builders.pad_masks([t["masks"] for t in targets])
    assert tuple(padded.shape) == (2, 3, 24, 28) and padded.dtype == torch.bool and not bool(padded[1, 2].any())
    assert not bool(padded[0, :, 20:].any()) and not bool(padded[1, :, :, 22:].any())


def test_patch_mask_losses_sets_and_restores_the_method_and_leaves_the_other_patches_alone():
    import devis_amd

    class TheirHead(torch.nn.Module):
        pass

    crit = types.SimpleNamespace(SetCriterion=type("SetCriterion", (StandInCriterion,), {}))
    seg = types.SimpleNamespace(MaskHeadConv=TheirHead, ModulatedDeformableConv2d=TheirHead, MultiScaleMHAttentionMap=TheirHead)
    theirs = crit.SetCriterion.loss_masks
    existing = crit.SetCriterion()
    previous = devis_amd.patch_mask_losses(crit)
    assert previous is theirs and crit.SetCriterion.loss_masks is devis_amd.argument_builders.loss_masks
    assert existing.loss_masks.__func__ is devis_amd.argument_builders.loss_masks      # criteria that exist follow
    assert (seg.MaskHeadConv, seg.ModulatedDeformableConv2d, seg.MultiScaleMHAttentionMap) == (TheirHead,) * 3
    devis_amd.unpatch_mask_losses(crit, previous)
    assert crit.SetCriterion.loss_masks is theirs and existing.loss_masks(None, None, None, None) == "theirs"
    before = crit.SetCriterion.loss_masks
    undo = devis_amd.patch_mask_head_stages(seg)        # another patch does not touch the criterion
    assert crit.SetCriterion.loss_masks is before
    devis_amd.unpatch_mask_head_stages(seg, undo)
    with pytest.raises(AttributeError):
        devis_amd.patch_mask_losses(types.SimpleNamespace())


# ---- fake-tensor paths -----------------------------------------------------------------------------------------------

def _nodes(graph):
    return [n for n in graph.nodes if n.op == "call_function" and "mask_loss_terms" in str(n.target)
            and "backward" not in str(n.target)]


def test_make_fx_with_fake_tensors_gives_one_op_node():
    from torch.fx.experimental.proxy_tensor import make_fx
    from devis_amd import ops
    meta = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")      # noqa: E731
    fn = lambda s, t: ops.mask_loss_terms_op(s, t, 0.25, 2.0)      # noqa: E731
    for dtype, acc in ((torch.float32, torch.float32), (torch.bfloat16, torch.float32), (torch.float64, torch.float64)):
        gm = make_fx(fn, tracing_mode="fake")(meta(5, 12, 20, dtype=dtype), meta(5, 45, 80, dtype=torch.bool))
        nodes = _nodes(gm.graph)
        assert len(nodes) == 1
        focal, dice, sums = nodes[0].meta["val"]
        assert tuple(focal.shape) == tuple(dice.shape) == (5,) and tuple(sums.shape) == (5, 3)
        assert focal.dtype == dice.dtype == sums.dtype == acc
    with pytest.raises(Exception, match="gamma"):
        make_fx(lambda s, t: ops.mask_loss_terms_op(s, t, 0.25, 0.5), tracing_mode="fake")(meta(5, 12, 20), meta(5, 45, 80))


@pytest.mark.parametrize("dynamic", [False, True])
def test_export_gives_one_op_node_for_static_and_dynamic_sizes(dynamic):
    import devis_amd

    class Wrap(torch.nn.Module):
        def forward(self, src, target):
            out = devis_amd.mask_losses(src, target, 3.0)
            return out["loss_mask"], out["loss_dice"]

    args = (torch.empty(5, 1, 12, 20, device="meta"), torch.empty(5, 45, 80, dtype=torch.bool, device="meta"))
    shapes = None
    if dynamic:
        D = torch.export.Dim
        N, h, w = D("N", min=2, max=512), D("h", min=2, max=512), D("w", min=2, max=512)
        H, W = D("H", min=2, max=2048), D("W", min=2, max=2048)
        shapes = ({0: N, 2: h, 3: w}, {0: N, 1: H, 2: W})
    ep = torch.export.export(Wrap(), args, dynamic_shapes=shapes)
    nodes = _nodes(ep.graph)
    assert len(nodes) == 1
    focal, dice, sums = nodes[0].meta["val"]
    assert len(focal.shape) == 1 and tuple(sums.shape)[1] == 3
    if dynamic:
        assert not isinstance(focal.shape[0], int)
    else:
        assert tuple(focal.shape) == (5,)
