"""CPU tests of the criterion's matching cost and box losses: the oracle against the reference fixtures and against torch
autograd, the C ABI of include/boxmatch.h (exports, version, argument errors -- no compute calls), the host code (shape checks,
errors, no backward call without a gradient to compute), the drop-ins of patch_criterion on stand-in matcher and criterion
classes with the operator replaced by the oracle, and the fake-tensor paths.  The kernels themselves are
tests/test_boxmatch_gpu.py."""
import ctypes
import os
import re
import types

import pytest
import torch

import boxmatch_oracle
from conftest import ROOT, golden, golden_names

FIXTURES = golden_names("boxmatch_")
F64 = torch.float64


def load_fixture(name):
    return {k: torch.from_numpy(v) for k, v in golden(name).items()}


def weights(d):
    return dict(cost_class=float(d["cost_class"]), cost_bbox=float(d["cost_bbox"]), cost_giou=float(d["cost_giou"]))


def close(got, want, tol=1e-12):
    return bool(((got - want).abs() <= tol * want.abs().clamp(min=1)).all())


def devis_operands(d):
    """(logits [1, F, Q, C], boxes [1, F, Q, 4], labels [T, F], tgt_boxes [T, F, 4]) of a DeVIS fixture."""
    Fr, Q, C, T = (int(v) for v in d["dims"])
    return (d["logits"].reshape(1, Fr, Q, C), d["boxes"].reshape(1, Fr, Q, 4), d["labels"].reshape(T, Fr),
            d["tgt_boxes"].reshape(T, Fr, 4))


def image_operands(d):
    B, Q, C = (int(v) for v in d["dims"])
    labels = torch.cat([d["labels_%d" % b] for b in range(B)])
    boxes = torch.cat([d["tgt_boxes_%d" % b] for b in range(B)])
    return d["logits"].reshape(1, 1, B * Q, C), d["boxes"].reshape(1, 1, B * Q, 4), labels.reshape(-1, 1), boxes.reshape(-1, 1, 4)


# ---- oracle ----------------------------------------------------------------------------------------------------------

def test_fixtures_cover_the_cases():
    assert FIXTURES == ["boxmatch_boxes", "boxmatch_devis_mean", "boxmatch_devis_sum", "boxmatch_image"]
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 32 << 10
    for name, use_sum in (("boxmatch_devis_mean", False), ("boxmatch_devis_sum", True)):
        d = load_fixture(name)
        assert d["dims"].tolist() == [3, 7, 5, 4] and bool(d["use_sum"]) == use_sum and float(d["margin"]) > 1e-2
        assert d["logits"].dtype == F64 and tuple(d["cost"].shape) == (7, 4)
        assert d["index_i"].dtype == d["index_j"].dtype == torch.int64 and d["index_valid"].dtype == torch.bool
        assert tuple(d["index_i"].shape) == (12,) and not bool(d["valid"].all()) and bool(d["valid"].any())
    d = load_fixture("boxmatch_image")
    assert d["dims"].tolist() == [2, 7, 5] and d["sizes"].tolist() == [3, 2] and float(d["margin"]) > 1e-2
    b = load_fixture("boxmatch_boxes")
    assert tuple(b["src"].shape) == (9, 4) and torch.equal(b["src"][0], b["target"][0]) and float(b["num_boxes"]) == 4.0


@pytest.mark.parametrize("name", ["boxmatch_devis_mean", "boxmatch_devis_sum"])
def test_oracle_equals_the_reference_devis_cost(name):
    d = load_fixture(name)
    cost, status = boxmatch_oracle.match_cost(*devis_operands(d), l1="sum" if bool(d["use_sum"]) else "mean",
                                              alpha=float(d["alpha"]), **weights(d))
    assert cost.dtype == F64 and tuple(cost.shape) == (1, 7, 4) and close(cost[0], d["cost"])
    assert status.dtype == torch.int32 and status.tolist() == [0, 0, 0]


def test_oracle_equals_the_reference_image_cost():
    d = load_fixture("boxmatch_image")
    cost, status = boxmatch_oracle.match_cost(*image_operands(d), l1="sum", alpha=float(d["alpha"]), **weights(d))
    cost = cost.reshape(2, 7, 5)
    assert close(cost[0, :, :3], d["cost_0"]) and close(cost[1, :, 3:], d["cost_1"]) and status.tolist() == [0, 0, 0]


def test_oracle_equals_the_reference_box_losses_and_gradient():
    d = load_fixture("boxmatch_boxes")
    lb, lg, grad = boxmatch_oracle.box_losses(d["src"], d["target"], float(d["num_boxes"]), with_grad=True)
    for got, want in ((lb, d["loss_bbox"]), (lg, d["loss_giou"]), (grad, d["grad_src"])):
        assert got.dtype == F64 and close(got, want)
    assert float(d["grad_src"][0, :2].abs().max()) == 0.0 and float(d["grad_src"][0, 2:].abs().min()) > 0      # the tie row


def tie_cases():
    """Rows that meet the non-smooth points: identical boxes, a shared left edge, touching boxes (the clamp at exactly 0),
    equal single coordinates (|0|), a box in a corner of the unit square.  Every number is a small dyadic fraction, so the
    corners are exact -- and the ties are ties -- in every arithmetic and storage type."""
    src = torch.tensor([[0.5, 0.5, 0.25, 0.375], [0.375, 0.5, 0.25, 0.5], [0.25, 0.5, 0.25, 0.25], [0.5, 0.375, 0.25, 0.25],
                        [0.25, 0.25, 0.5, 0.5]], dtype=F64)
    tgt = torch.tensor([[0.5, 0.5, 0.25, 0.375], [0.4375, 0.5, 0.375, 0.5], [0.5, 0.5, 0.25, 0.25], [0.5, 0.625, 0.25, 0.125],
                        [0.5, 0.5, 1.0, 1.0]], dtype=F64)
    return src, tgt


def test_oracle_gradient_is_torch_autograds_also_at_the_ties():
    g = torch.Generator().manual_seed(11)
    rnd = torch.rand(6, 4, generator=g, dtype=F64) * 0.4 + 0.2
    src, tgt = tie_cases()
    src, tgt = torch.cat([src, rnd]), torch.cat([tgt, rnd.flip(0)])
    g1, gg = torch.randn(11, generator=g, dtype=F64), torch.randn(11, generator=g, dtype=F64)
    l1, gl, grad = boxmatch_oracle.box_loss_terms(src, tgt, grads=(g1, gg))
    s = src.clone().requires_grad_(True)
    want_l1, want_gl = (s - tgt).abs().sum(-1), 1 - boxmatch_oracle.giou(s, tgt)
    want, = torch.autograd.grad((want_l1 * g1).sum() + (want_gl * gg).sum(), s)
    assert close(l1, want_l1.detach()) and close(gl, want_gl.detach()) and close(grad, want)
    # identical boxes: the halves of the centre's gradient cancel; the sides keep what the 1e-6 terms leave
    assert float(grad[0, :2].abs().max()) <= 1e-12 and 0 < float(grad[0, 2:].abs().min()) < 1e-3


def test_oracle_class_cost_follows_the_formula_and_stays_finite():
    x = torch.tensor([-30.0, -3.0, 0.0, 3.0, 30.0, float("inf"), -float("inf")], dtype=F64)
    got = boxmatch_oracle.class_cost(x, 0.25)
    assert bool(torch.isfinite(got).all())
    p = torch.sigmoid(x[1:4])
    want = 0.25 * (1 - p) ** 2 * (-(p + 1e-8).log()) - 0.75 * p ** 2 * (-(1 - p + 1e-8).log())
    assert close(got[1:4], want)
    assert abs(float(got[4]) + 0.75 * 18.420680743952367) < 1e-4 and abs(float(got[0]) - 0.25 * 18.420680743952367) < 1e-4


def test_oracle_status_and_nan_for_bad_labels_and_degenerate_boxes():
    d = load_fixture("boxmatch_devis_mean")
    logits, boxes, labels, tgt = (t.clone() for t in devis_operands(d))
    labels[2, 1] = 5
    labels[0, 0] = -1
    tgt[1, 2, 2] = -0.1
    boxes[0, 1, 3, 3] = -0.2
    boxes[0, 1, 4, 2] = -0.2
    cost, status = boxmatch_oracle.match_cost(logits, boxes, labels, tgt)
    assert status.tolist() == [2, 1, 2]
    assert bool(torch.isnan(cost[0, :, 2]).all()) and bool(torch.isnan(cost[0, :, 0]).all()) and bool(torch.isfinite(cost[0, :, 3]).all())


# ---- library ---------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_boxmatch_h_declares_and_versions_agree():
    from devis_amd import _boxmatch, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "boxmatch.h")).read()
    declared = set(re.findall(r"\b(boxmatch_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_boxmatch.EXPORTED_SYMBOLS) and len(declared) == 5
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _boxmatch.load()
    assert lib.boxmatch_version() == _boxmatch.BOXMATCH_ABI_VERSION == int(re.search(r"#define BOXMATCH_ABI_VERSION (\d+)", header).group(1))
    assert dict(re.findall(r"BOXMATCH_(F32|F64|BF16|F16) = (\d)", header)) == {"F32": "0", "F64": "1", "BF16": "2", "F16": "3"}
    kinds = dict(re.findall(r"BOXMATCH_TARGET_(SAME|F32) = (\d)", header))
    assert kinds == {"SAME": str(_boxmatch.TARGET_SAME), "F32": str(_boxmatch.TARGET_F32)}
    assert dict(re.findall(r"BOXMATCH_L1_(MEAN|SUM) = (\d)", header)) == {"MEAN": str(_boxmatch.L1_MEAN), "SUM": str(_boxmatch.L1_SUM)}
    for stated in ("half of the gradient", "v == 0 included", "derivative 0 at v == 0"):      # the ties are stated
        assert stated in header
    assert os.path.join(build.include_dir(), "boxmatch.h") in build._headers()
    assert any(s.endswith("boxmatch.hip") for s in build.sources())
    assert "boxmatch.h" in open(os.path.join(ROOT, "setup.py")).read()


def test_boxmatch_argument_errors_without_gpu():
    from devis_amd import _boxmatch
    lib = _boxmatch.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    shape = lambda **kw: ctypes.byref(_boxmatch.Shape(**dict(dict(L=1, F=3, R=7, T=4, C=5), **kw)))      # noqa: E731
    err = lib.boxmatch_last_error

    def cost(dtype=0, kind=0, logits=p, boxes=p, labels=p, tgt=p, shape=shape(), wc=1.0, wb=1.0, wg=1.0, l1=0, alpha=0.25,
             out=p, status=p):
        return lib.boxmatch_cost(dtype, kind, logits, boxes, labels, tgt, shape, wc, wb, wg, l1, alpha, out, status, None)

    def fwd(dtype=0, kind=0, src=p, tgt=p, N=3, l1=p, giou=p):
        return lib.boxmatch_loss_forward(dtype, kind, src, tgt, N, l1, giou, None)

    def bwd(dtype=0, kind=0, src=p, tgt=p, g1=p, gg=p, N=3, gs=p):
        return lib.boxmatch_loss_backward(dtype, kind, src, tgt, g1, gg, N, gs, None)

    for call in (cost, fwd, bwd):
        assert call(dtype=9) == -1 and b"dtype" in err()
        assert call(dtype=-1) == -1 and b"dtype" in err()
        assert call(kind=2) == -1 and b"target kind" in err()
        assert call(dtype=1, kind=1) == -1 and b"target kind" in err()      # float32 targets beside float64
        for name in ("src", "tgt") if call is not cost else ("logits", "boxes", "labels", "tgt", "out", "status"):
            assert call(**{name: None}) == -1 and b"null pointer" in err(), name
    assert cost(shape=None) == -1 and b"null pointer" in err()
    assert cost(l1=2) == -1 and b"l1" in err()
    assert cost(alpha=float("nan")) == -1 and b"NaN" in err()
    for bad in (dict(F=0), dict(C=0), dict(F=-1)):
        assert cost(shape=shape(**bad)) == -1 and b"positive" in err(), bad
    for bad in (dict(L=-1), dict(R=-1), dict(T=-1)):
        assert cost(shape=shape(**bad)) == -1 and b"negative" in err(), bad
    assert cost(shape=shape(L=2048, R=2048, T=2048)) == -1 and b"31 bits" in err()
    for name in ("l1", "giou"):
        assert fwd(**{name: None}) == -1 and b"null pointer" in err(), name
    for name in ("g1", "gg", "gs"):
        assert bwd(**{name: None}) == -1 and b"null pointer" in err(), name
    assert fwd(N=-1) == -1 and bwd(N=-1) == -1 and b"negative" in err()
    # nothing to compute: nothing is launched, nothing is dereferenced
    for empty in (dict(L=0), dict(R=0), dict(T=0)):
        assert cost(logits=None, boxes=None, labels=None, tgt=None, out=None, status=None, shape=shape(**empty)) == 0
    assert fwd(src=None, tgt=None, l1=None, giou=None, N=0) == 0
    assert bwd(src=None, tgt=None, g1=None, gg=None, gs=None, N=0) == 0


# ---- host ------------------------------------------------------------------------------------------------------------

def test_operators_raise_on_cpu_tensors_and_on_bad_arguments_before_any_launch(monkeypatch):
    import devis_amd
    from devis_amd import _boxmatch
    from devis_amd.functions import box_matching as X

    def no_launch(*a, **k):
        raise AssertionError("a kernel call was made")

    for name in ("cost", "loss_forward", "loss_backward"):
        monkeypatch.setattr(_boxmatch, name, no_launch)
    logits, boxes = torch.zeros(1, 3, 7, 5), torch.zeros(1, 3, 7, 4)
    labels, tgt = torch.zeros(4, 3, dtype=torch.int64), torch.zeros(4, 3, 4)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.match_cost(logits, boxes, labels, tgt)
    with pytest.raises(ValueError, match="l1 must be 'mean' or 'sum'"):
        devis_amd.match_cost(logits, boxes, labels, tgt, l1="max")
    with pytest.raises(RuntimeError, match="match_cost: logits requires a gradient"):
        devis_amd.match_cost(logits.clone().requires_grad_(True), boxes, labels, tgt)
    with torch.no_grad(), pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.match_cost(logits.clone().requires_grad_(True), boxes, labels, tgt)
    src, target = torch.zeros(3, 4), torch.zeros(3, 4)
    for fn in (devis_amd.box_loss_terms, lambda s, t: devis_amd.box_losses(s, t, 3.0)):
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            fn(src, target)
        with pytest.raises(RuntimeError, match="no gradient"):
            fn(src, target.clone().requires_grad_(True))
        with pytest.raises(RuntimeError, match="target_boxes must be \\[N, 4\\] like src_boxes"):
            fn(src, torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        X._backward(torch.zeros(3), torch.zeros(3), src, target)
    for name in ("match_cost", "box_loss_terms", "box_losses", "patch_criterion", "unpatch_criterion"):
        assert name in devis_amd.__all__ and getattr(devis_amd, name) is getattr(
            devis_amd.ops if "patch" not in name else devis_amd.argument_builders, name)

    meta = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="meta")      # noqa: E731
    h, i64 = torch.bfloat16, torch.int64
    ok = (meta(2, 3, 7, 5), meta(2, 3, 7, 4), meta(4, 3, dtype=i64), meta(4, 3, 4))
    assert X.check_match(*ok) == (2, 3, 7, 4, 5, _boxmatch.TARGET_SAME)
    assert X.check_match(meta(2, 3, 7, 5, dtype=h), meta(2, 3, 7, 4, dtype=h), ok[2], ok[3])[-1] == _boxmatch.TARGET_F32
    assert X.check_match(meta(0, 3, 7, 5), meta(0, 3, 7, 4), meta(0, 3, dtype=i64), meta(0, 3, 4))[:4] == (0, 3, 7, 0)
    assert X.check_pairs(meta(6, 4), meta(6, 4)) == (6, _boxmatch.TARGET_SAME)
    assert X.check_pairs(meta(6, 4, dtype=torch.float16), meta(6, 4)) == (6, _boxmatch.TARGET_F32)
    bad = [
        ("logits must be \\[L, F, R, C\\]", lambda: X.check_match(meta(3, 7, 5), *ok[1:])),
        ("boxes must be \\[L, F, R, 4\\]", lambda: X.check_match(ok[0], meta(2, 3, 6, 4), *ok[2:])),
        ("logits is torch.float32, boxes is torch.float64", lambda: X.check_match(ok[0], meta(2, 3, 7, 4, dtype=F64), *ok[2:])),
        ("unsupported dtype", lambda: X.check_match(meta(2, 3, 7, 5, dtype=torch.int32), *ok[1:])),
        ("tgt_labels must be int64", lambda: X.check_match(ok[0], ok[1], meta(4, 3, dtype=torch.int32), ok[3])),
        ("tgt_labels has 2 frames, logits 3", lambda: X.check_match(ok[0], ok[1], meta(4, 2, dtype=i64), ok[3])),
        ("tgt_boxes must be \\[T, F, 4\\]", lambda: X.check_match(*ok[:3], meta(5, 3, 4))),
        ("tgt_boxes must be of the predictions' dtype", lambda: X.check_match(*ok[:3], meta(4, 3, 4, dtype=F64))),
        ("no frames or no classes", lambda: X.check_match(meta(2, 0, 7, 5), meta(2, 0, 7, 4), meta(4, 0, dtype=i64), meta(4, 0, 4))),
        ("src_boxes must be \\[N, 4\\]", lambda: X.check_pairs(meta(6, 3), meta(6, 3))),
        ("target_boxes must be of the predictions' dtype", lambda: X.check_pairs(meta(6, 4), meta(6, 4, dtype=h))),
    ]
    for match, call in bad:
        with pytest.raises(RuntimeError, match=match):
            call()


def test_no_backward_call_when_src_needs_no_gradient():
    from devis_amd import ops
    from devis_amd.functions import box_matching as X
    seen = []
    src, target, g1, gg = torch.zeros(3, 4), torch.zeros(3, 4), torch.ones(3), torch.ones(3)
    host = lambda *a: seen.append("host") or torch.zeros(3, 4)      # noqa: E731
    op = lambda *a: seen.append("op") or torch.zeros(3, 4)      # noqa: E731
    # the one formula, run the way the eager Function runs it and the way the op's register_autograd does
    assert X.BoxLossTermsFunction.setup_context is X.setup_context is ops.box_loss_terms_op._setup_context_fn
    assert ops.box_loss_terms_op._backward_fn.func is X.backward
    for needs in ((False, False), (True, False)):
        ctx = types.SimpleNamespace(saved_tensors=(src, target), needs_input_grad=needs)
        before = len(seen)
        for res in (X.backward(host, ctx, g1, gg), X.backward(op, ctx, g1, gg)):
            assert len(res) == 2 and res[1] is None and (res[0] is None) == (not needs[0])
        assert seen[before:] == (["host", "op"] if needs[0] else [])


# ---- the drop-ins of patch_criterion -------------------------------------------------------------------------------------

class StandInDeVISMatcher(torch.nn.Module):
    """The attributes the reference's DeVISHungarianMatcher carries; its own ``forward`` is a marker."""

    def __init__(self, d, focal_loss=True):
        super().__init__()
        Fr, Q = int(d["dims"][0]), int(d["dims"][1])
        self.cost_class, self.cost_bbox, self.cost_giou = (float(d[k]) for k in ("cost_class", "cost_bbox", "cost_giou"))
        self.num_frames, self.num_out, self.focal_loss, self.focal_alpha = Fr, Q, focal_loss, float(d["alpha"])
        self.use_l1_distance_sum = bool(d["use_sum"]) if "use_sum" in d else False

    def forward(self, outputs, targets):
        return "theirs"


class StandInImageMatcher(torch.nn.Module):
    def __init__(self, d, focal_loss=True):
        super().__init__()
        self.cost_class, self.cost_bbox, self.cost_giou = (float(d[k]) for k in ("cost_class", "cost_bbox", "cost_giou"))
        self.focal_loss, self.focal_alpha = focal_loss, float(d["alpha"])

    def forward(self, outputs, targets):
        return "theirs"


class StandInCriterion:
    """What the drop-ins need of a criterion: the index helpers, and a ``forward`` that honours ``"indices"`` as the
    reference's does (the suite's restatement: it returns the matchings it used, top level first)."""

    def __init__(self, matcher=None):
        self.matcher = matcher

    @staticmethod
    def _cat(indices, masked):
        batch = torch.cat([torch.full_like(e[0], i)[e[2]] if masked else torch.full_like(e[0], i) for i, e in enumerate(indices)])
        return batch, torch.cat([e[0][e[2]] if masked else e[0] for e in indices])

    def _get_src_permutation_idx(self, indices, from_devis=False):
        assert from_devis == (len(indices[0]) == 3)
        return self._cat(indices, False)

    def _get_src_permutation_masked_idx(self, indices):
        return self._cat(indices, True)

    def loss_boxes(self, outputs, targets, indices, num_boxes):
        return "theirs"

    def forward(self, outputs, targets):
        used = [outputs["indices"] if "indices" in outputs else self.matcher({k: v for k, v in outputs.items() if k != "aux_outputs"}, targets)]
        for aux in outputs.get("aux_outputs", ()):
            used.append(aux["indices"] if "indices" in aux else self.matcher(aux, targets))
        return used


def modules():
    crit = types.SimpleNamespace(SetCriterion=type("SetCriterion", (StandInCriterion,), {}))
    match = types.SimpleNamespace(DeVISHungarianMatcher=type("DeVISHungarianMatcher", (StandInDeVISMatcher,), {}),
                                  HungarianMatcher=type("HungarianMatcher", (StandInImageMatcher,), {}))
    return crit, match


@pytest.fixture()
def patched(monkeypatch):
    """(criterion module, matcher module) with patch_criterion applied and the operator replaced by the oracle, which counts
    its calls in ``calls``."""
    import devis_amd
    from devis_amd import ops
    crit, match = modules()
    calls = []

    def oracle_cost(*a, **k):
        calls.append(tuple(a[0].shape))
        return boxmatch_oracle.match_cost(*a, **k)

    monkeypatch.setattr(ops, "match_cost", oracle_cost)
    previous = devis_amd.patch_criterion(crit, match)
    yield crit, match, calls
    devis_amd.unpatch_criterion(crit, match, previous)


def devis_call(d):
    return ({"pred_logits": d["logits"], "pred_boxes": d["boxes"]},
            [{"labels": d["labels"], "boxes": d["tgt_boxes"], "valid": d["valid"]}])


def image_call(d):
    return ({"pred_logits": d["logits"], "pred_boxes": d["boxes"]},
            [{"labels": d["labels_%d" % b], "boxes": d["tgt_boxes_%d" % b]} for b in range(2)])


def same_tensors(got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and g.device == w.device and torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("name", ["boxmatch_devis_mean", "boxmatch_devis_sum"])
def test_patched_devis_matcher_returns_the_reference_indices(name, patched):
    crit, match, calls = patched
    d = load_fixture(name)
    out = match.DeVISHungarianMatcher(d)(*devis_call(d))
    assert isinstance(out, list) and len(out) == 1 and isinstance(out[0], tuple)
    assert same_tensors(out[0], (d["index_i"], d["index_j"], d["index_valid"])) and calls == [(1, 3, 7, 5)]
    # a second batch element is never looked at, as in the reference (it returns inside its loop)
    outputs, targets = devis_call(d)
    two = {k: torch.cat([v, v.flip(1)]) for k, v in outputs.items()}
    out2 = match.DeVISHungarianMatcher(d)(two, targets + [{"labels": None}])
    assert len(out2) == 1 and same_tensors(out2[0], out[0])
    assert match.DeVISHungarianMatcher(d, focal_loss=False)(*devis_call(d)) == "theirs"       # the non-focal path is theirs


def test_patched_image_matcher_returns_the_reference_indices(patched):
    crit, match, calls = patched
    d = load_fixture("boxmatch_image")
    out = match.HungarianMatcher(d)(*image_call(d))
    assert len(out) == 2 and calls == [(1, 1, 14, 5)]
    for b, pair in enumerate(out):
        assert isinstance(pair, tuple) and same_tensors(pair, (d["index_i_%d" % b], d["index_j_%d" % b]))
    assert match.HungarianMatcher(d, focal_loss=False)(*image_call(d)) == "theirs"
    # an image without targets: an empty matching for it, the other one as before
    outputs, targets = image_call(d)
    targets[0] = {"labels": targets[0]["labels"][:0], "boxes": targets[0]["boxes"][:0]}
    out = match.HungarianMatcher(d)(outputs, targets)
    assert out[0][0].numel() == 0 and out[0][0].dtype == torch.int64 and same_tensors(out[1], (d["index_i_1"], d["index_j_1"]))


def test_patched_matchers_raise_what_the_reference_raises(patched):
    crit, match, calls = patched
    d = load_fixture("boxmatch_devis_mean")
    outputs, targets = devis_call(d)
    bad = dict(targets[0], labels=targets[0]["labels"].clone())
    bad["labels"][4] = 5
    with pytest.raises(IndexError, match="outside \\[0, 5\\)"):
        match.DeVISHungarianMatcher(d)(outputs, [bad])
    bad = dict(targets[0], boxes=targets[0]["boxes"].clone())
    bad["boxes"][3, 2] = -0.1
    with pytest.raises(AssertionError, match="1 target box"):
        match.DeVISHungarianMatcher(d)(outputs, [bad])
    worse = dict(outputs, pred_boxes=outputs["pred_boxes"].clone())
    worse["pred_boxes"][0, 5, 3] = -0.1
    with pytest.raises(AssertionError, match="1 prediction"):
        match.DeVISHungarianMatcher(d)(worse, targets)


def test_a_clip_without_targets_gets_the_reference_triple_without_any_launch(patched):
    crit, match, calls = patched
    d = load_fixture("boxmatch_devis_mean")
    outputs, targets = devis_call(d)
    none = [{"labels": targets[0]["labels"][:2], "boxes": targets[0]["boxes"][:2], "valid": targets[0]["valid"][:2]}]    # 2 // 3 == 0
    (index_i, index_j, index_valid), = match.DeVISHungarianMatcher(d)(outputs, none)
    assert calls == []
    assert same_tensors((index_i, index_j, index_valid), (torch.arange(3) * 7, torch.arange(3), torch.zeros(3, dtype=torch.bool)))


@pytest.mark.parametrize("kind", ["devis", "image"])
def test_batch_aux_yields_the_per_call_indices_with_one_cost_call_and_leaves_the_dicts_alone(kind, monkeypatch):
    import devis_amd
    from devis_amd import ops
    crit, match = modules()
    calls = []
    monkeypatch.setattr(ops, "match_cost", lambda *a, **k: calls.append(tuple(a[0].shape)) or boxmatch_oracle.match_cost(*a, **k))
    d = load_fixture("boxmatch_devis_mean" if kind == "devis" else "boxmatch_image")
    top, targets = devis_call(d) if kind == "devis" else image_call(d)
    g = torch.Generator().manual_seed(3)
    layer = lambda: {"pred_logits": top["pred_logits"] + 0.5 * torch.randn(top["pred_logits"].shape, generator=g, dtype=F64),      # noqa: E731
                     "pred_boxes": top["pred_boxes"] * (1 + 0.1 * torch.rand(top["pred_boxes"].shape, generator=g, dtype=F64))}
    matcher = (match.DeVISHungarianMatcher if kind == "devis" else match.HungarianMatcher)(d)
    given = ["given"]
    outputs = dict(top, aux_outputs=[layer(), dict(layer(), indices=given), layer()])
    keys = [sorted(outputs)] + [sorted(a) for a in outputs["aux_outputs"]]

    previous = devis_amd.patch_criterion(crit, match)
    try:
        per_call = crit.SetCriterion(matcher).forward(outputs, targets)
    finally:
        devis_amd.unpatch_criterion(crit, match, previous)
    assert len(calls) == 3 and per_call[2] is given
    del calls[:]
    previous = devis_amd.patch_criterion(crit, match, batch_aux=True)
    try:
        assert "criterion_forward" in previous
        existing = crit.SetCriterion(matcher)
        batched = existing.forward(outputs, targets)
        lead = (3, 3, 7, 5) if kind == "devis" else (3, 1, 14, 5)
        assert calls == [lead]                                                                  # one cost call for three dicts
        assert [sorted(outputs)] + [sorted(a) for a in outputs["aux_outputs"]] == keys          # nothing was added to the caller's
        assert len(batched) == 4 and batched[2] is given
        for got, want in zip(batched[:2] + batched[3:], per_call[:2] + per_call[3:]):
            assert len(got) == len(want) and all(same_tensors(a, b) for a, b in zip(got, want))
        assert same_tensors(batched[0][0], (d["index_i"], d["index_j"], d["index_valid"]) if kind == "devis"
                            else (d["index_i_0"], d["index_j_0"]))
        # another matcher class, or the non-focal path: straight through
        del calls[:]
        other = crit.SetCriterion(torch.nn.Identity())
        other.matcher = lambda o, t: "other"
        assert other.forward(outputs, targets) == ["other", "other", given, "other"] and calls == []
        matcher.focal_loss = False
        assert existing.forward(outputs, targets) == ["theirs", "theirs", given, "theirs"] and calls == []
    finally:
        devis_amd.unpatch_criterion(crit, match, previous)
    assert crit.SetCriterion.forward is StandInCriterion.forward


@pytest.mark.parametrize("form", ["image", "devis", "devis_masked"])
def test_loss_boxes_selects_the_reference_boxes_for_two_and_three_tuples(form, monkeypatch):
    from devis_amd import argument_builders, ops
    g = torch.Generator().manual_seed(2)
    pred = torch.rand(2, 6, 4, generator=g)
    targets = [{"boxes": torch.rand(3, 4, generator=g)}, {"boxes": torch.rand(2, 4, generator=g, dtype=F64)[:, :4].float()}]
    src_i, tgt_j = [torch.tensor([4, 1]), torch.tensor([0, 3])], [torch.tensor([2, 0]), torch.tensor([1, 0])]
    chosen = [(0, 4, 2), (0, 1, 0), (1, 0, 1), (1, 3, 0)]
    if form == "image":
        indices = [(src_i[0], tgt_j[0]), (src_i[1], tgt_j[1])]
    elif form == "devis":
        indices = [(src_i[0], tgt_j[0], torch.tensor([True, False])), (src_i[1], tgt_j[1], torch.tensor([True, True]))]
    else:       # the first clip's mask selects nothing: every clip is masked
        indices = [(src_i[0], tgt_j[0], torch.tensor([False, False])), (src_i[1], tgt_j[1], torch.tensor([False, True]))]
        chosen = [(1, 3, 0)]
    seen = {}
    monkeypatch.setattr(ops, "box_losses", lambda s, t, n: seen.update(src=s, target=t, num_boxes=n) or {"loss_bbox": 1, "loss_giou": 2})
    assert argument_builders.loss_boxes(StandInCriterion(), {"pred_boxes": pred}, targets, indices, 3.5) == {"loss_bbox": 1, "loss_giou": 2}
    assert torch.equal(seen["src"], torch.stack([pred[b, q] for b, q, _ in chosen]))
    assert torch.equal(seen["target"], torch.stack([targets[b]["boxes"][j] for b, _, j in chosen])) and seen["num_boxes"] == 3.5


def test_patch_criterion_sets_and_restores_the_methods_and_leaves_the_other_patches_alone():
    import devis_amd
    crit, match = modules()
    crit.SetCriterion.loss_masks = lambda self, *a: "their masks"
    theirs = (crit.SetCriterion.loss_boxes, crit.SetCriterion.forward, crit.SetCriterion.loss_masks,
              match.DeVISHungarianMatcher.forward, match.HungarianMatcher.forward)
    current = lambda: (crit.SetCriterion.loss_boxes, crit.SetCriterion.forward, crit.SetCriterion.loss_masks,      # noqa: E731
                       match.DeVISHungarianMatcher.forward, match.HungarianMatcher.forward)
    existing = crit.SetCriterion()
    previous = devis_amd.patch_criterion(crit, match)
    assert previous == {"loss_boxes": theirs[0], "devis_forward": theirs[3], "image_forward": theirs[4]}
    assert crit.SetCriterion.loss_boxes is devis_amd.argument_builders.loss_boxes
    assert existing.loss_boxes.__func__ is devis_amd.argument_builders.loss_boxes             # criteria that exist follow
    now = current()
    assert now[1] is theirs[1] and now[2] is theirs[2] and now[3] is not theirs[3] and now[4] is not theirs[4]
    undo = devis_amd.patch_mask_losses(crit)                    # independent of the mask-loss patch, in either order
    devis_amd.unpatch_criterion(crit, match, previous)
    assert crit.SetCriterion.loss_masks is devis_amd.argument_builders.loss_masks and crit.SetCriterion.loss_boxes is theirs[0]
    devis_amd.unpatch_mask_losses(crit, undo)
    assert current() == theirs and existing.loss_boxes(None, None, None, None) == "theirs"
    previous = devis_amd.patch_criterion(crit, match, batch_aux=True)
    assert previous["criterion_forward"] is theirs[1] and crit.SetCriterion.forward is not theirs[1]
    devis_amd.unpatch_criterion(crit, match, previous)
    assert current() == theirs
    with pytest.raises(AttributeError):
        devis_amd.patch_criterion(types.SimpleNamespace(), match)
    assert current() == theirs


# ---- fake-tensor paths -----------------------------------------------------------------------------------------------

def _nodes(graph, name):
    return [n for n in graph.nodes if n.op == "call_function" and name in str(n.target) and "backward" not in str(n.target)]


def test_make_fx_with_fake_tensors_gives_one_op_node_each():
    from torch.fx.experimental.proxy_tensor import make_fx
    from devis_amd import ops
    meta = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")      # noqa: E731
    for dtype, acc in ((torch.float32, torch.float32), (torch.bfloat16, torch.float32), (F64, F64)):
        fn = lambda x, b, l, t: ops.match_cost_op(x, b, l, t, 2.0, 5.0, 2.0, "sum", 0.25)      # noqa: E731
        gm = make_fx(fn, tracing_mode="fake")(meta(6, 3, 7, 5, dtype=dtype), meta(6, 3, 7, 4, dtype=dtype),
                                              meta(4, 3, dtype=torch.int64), meta(4, 3, 4, dtype=dtype))
        node, = _nodes(gm.graph, "match_cost")
        cost, status = node.meta["val"]
        assert tuple(cost.shape) == (6, 7, 4) and cost.dtype == acc and tuple(status.shape) == (3,) and status.dtype == torch.int32
        gm = make_fx(ops.box_loss_terms_op, tracing_mode="fake")(meta(9, 4, dtype=dtype), meta(9, 4, dtype=dtype))
        node, = _nodes(gm.graph, "box_loss_terms")
        l1, giou = node.meta["val"]
        assert tuple(l1.shape) == tuple(giou.shape) == (9,) and l1.dtype == giou.dtype == acc
    with pytest.raises(Exception, match="l1 must be"):
        make_fx(lambda x, b, l, t: ops.match_cost_op(x, b, l, t, 1.0, 1.0, 1.0, "max", 0.25), tracing_mode="fake")(
            meta(6, 3, 7, 5), meta(6, 3, 7, 4), meta(4, 3, dtype=torch.int64), meta(4, 3, 4))


@pytest.mark.parametrize("dynamic", [False, True])
def test_export_gives_one_op_node_each_for_static_and_dynamic_sizes(dynamic):
    import devis_amd

    class Cost(torch.nn.Module):
        def forward(self, logits, boxes, labels, tgt):
            return devis_amd.match_cost(logits, boxes, labels, tgt, cost_class=2.0, l1="sum")

    class Loss(torch.nn.Module):
        def forward(self, src, target):
            out = devis_amd.box_losses(src, target, 3.0)
            return out["loss_bbox"], out["loss_giou"]

    D = torch.export.Dim
    args = (torch.empty(2, 3, 7, 5, device="meta"), torch.empty(2, 3, 7, 4, device="meta"),
            torch.empty(4, 3, dtype=torch.int64, device="meta"), torch.empty(4, 3, 4, device="meta"))
    shapes = None
    if dynamic:
        R, T = D("R", min=2, max=4096), D("T", min=2, max=256)
        shapes = ({2: R}, {2: R}, {0: T}, {0: T})
    node, = _nodes(torch.export.export(Cost(), args, dynamic_shapes=shapes).graph, "match_cost")
    cost = node.meta["val"][0]
    assert len(cost.shape) == 3 and cost.shape[0] == 2 and (not isinstance(cost.shape[1], int) if dynamic else tuple(cost.shape) == (2, 7, 4))
    args = (torch.empty(9, 4, device="meta"), torch.empty(9, 4, device="meta"))
    shapes = ({0: D("N", min=2, max=4096)},) * 2 if dynamic else None
    node, = _nodes(torch.export.export(Loss(), args, dynamic_shapes=shapes).graph, "box_loss_terms")
    l1 = node.meta["val"][0]
    assert len(l1.shape) == 1 and (not isinstance(l1.shape[0], int) if dynamic else tuple(l1.shape) == (9,))
