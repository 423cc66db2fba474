"""CPU tests of the criterion's label loss: the oracle against the reference fixtures, the C ABI of include/labelloss.h
(exports, version, argument errors -- no compute calls), the host code (shape checks, errors), the drop-in of patch_label_loss
on stand-in criterion classes with the operator replaced by the oracle, and the fake-tensor paths.  The kernels themselves
are tests/test_labelloss_gpu.py."""
import ctypes
import os
import re
import types

import pytest
import torch

import labelloss_oracle
from conftest import ROOT, golden, golden_names
from test_boxmatch_cpu import StandInCriterion, modules

FIXTURES = golden_names("labelloss_")
F64 = torch.float64


def load_fixture(name):
    return {k: torch.from_numpy(v) for k, v in golden(name).items()}


def close(got, want, tol=1e-10):
    return bool(((got - want).abs() <= tol * want.abs().clamp(min=1)).all())


def fixture_call(d):
    """(outputs, targets, indices, num_boxes) as the criterion hands them to loss_labels_focal."""
    if "index_valid" in d:
        return ({"pred_logits": d["logits"]}, [{"labels": d["labels"], "valid": d["valid"]}],
                [(d["index_i"], d["index_j"], d["index_valid"])], float(d["num_boxes"]))
    B = int(d["dims"][0])
    return ({"pred_logits": d["logits"]}, [{"labels": d["labels_%d" % b]} for b in range(B)],
            [(d["index_i_%d" % b], d["index_j_%d" % b]) for b in range(B)], float(d["num_boxes"]))


def fixture_operands(d):
    """(logits [B, N, C], rows [M], labels [M], valid [M] or None) of a fixture: the operator's operands."""
    outputs, targets, indices, _ = fixture_call(d)
    N = d["logits"].shape[1]
    rows = torch.cat([e[0] + i * N for i, e in enumerate(indices)])
    labels = torch.cat([t["labels"][e[1]] for t, e in zip(targets, indices)])
    valid = torch.cat([e[2] for e in indices]) if len(indices[0]) == 3 else None
    return d["logits"], rows, labels, valid


class StandInLabelCriterion(StandInCriterion):
    """What loss_labels_focal needs of a criterion: focal_alpha; its own method is a marker."""
    focal_alpha = 0.25

    def loss_labels_focal(self, outputs, targets, indices, num_boxes, log=True):
        return "theirs"


def label_modules():
    crit, match = modules()
    crit.SetCriterion = type("SetCriterion", (StandInLabelCriterion,), {})
    return crit, match


# ---- library ---------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_labelloss_h_declares_and_versions_agree():
    from devis_amd import _labelloss, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "labelloss.h")).read()
    declared = set(re.findall(r"\b(labelloss_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_labelloss.EXPORTED_SYMBOLS) and len(declared) == 6
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _labelloss.load()
    assert lib.labelloss_version() == _labelloss.LABELLOSS_ABI_VERSION == int(re.search(r"#define LABELLOSS_ABI_VERSION (\d+)", header).group(1))
    assert dict(re.findall(r"LABELLOSS_(F32|F64|BF16|F16) = (\d)", header)) == {"F32": "0", "F64": "1", "BF16": "2", "F16": "3"}
    assert int(re.search(r"#define LABELLOSS_TILE_ELEMENTS (\d+)", header).group(1)) == _labelloss.TILE_ELEMENTS
    assert _labelloss.tile() > 0 and lib.labelloss_tile(7) == -1 and lib.labelloss_tile(-1) == -1
    for stated in ("HIGHEST m", "LOWEST class index", "contains a NaN is never correct", "scanning all M matches is deliberate"):
        assert stated in re.sub(r"\s*\n \*\s*", " ", header), stated                      # the rules are stated
    assert os.path.join(build.include_dir(), "labelloss.h") in build._headers()
    assert any(s.endswith("labelloss.hip") for s in build.sources())
    assert "labelloss.h" in open(os.path.join(ROOT, "setup.py")).read() and "labelloss.h" in build.include_dir.__doc__


def test_labelloss_argument_errors_without_gpu():
    from devis_amd import _labelloss
    lib = _labelloss.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    shape = lambda **kw: ctypes.byref(_labelloss.Shape(**dict(dict(R=21, C=5, M=6), **kw)))      # noqa: E731
    err = lib.labelloss_last_error

    def fwd(dtype=0, logits=p, rows=p, labels=p, valid=p, shape=shape(), alpha=0.25, ws=p, tc=p, fs=p, counts=p):
        return lib.labelloss_forward(dtype, logits, rows, labels, valid, shape, alpha, ws, tc, fs, counts, None)

    def bwd(dtype=0, logits=p, tc=p, gs=p, shape=shape(), alpha=0.25, gl=p):
        return lib.labelloss_backward(dtype, logits, tc, gs, shape, alpha, gl, None)

    for call in (fwd, bwd):
        assert call(dtype=9) == -1 and b"dtype" in err()
        assert call(dtype=-1) == -1 and b"dtype" in err()
        assert call(shape=None) == -1 and b"null pointer" in err()
        assert call(alpha=float("nan")) == -1 and b"alpha" in err()
        for bad in (dict(R=-1), dict(C=-1), dict(M=-1)):
            assert call(shape=shape(**bad)) == -1 and b"negative" in err(), bad
        assert call(shape=shape(R=1 << 20, C=1 << 11)) == -1 and b"31 bits" in err()
    for name in ("logits", "rows", "labels", "tc", "fs", "counts"):
        assert fwd(**{name: None}) == -1 and b"null pointer" in err(), name
    for name in ("logits", "tc", "gs", "gl"):
        assert bwd(**{name: None}) == -1 and b"null pointer" in err(), name
    rows_per_tile = _labelloss.tile() // 5
    assert fwd(ws=None, shape=shape(R=rows_per_tile + 1)) == -1 and b"workspace" in err()       # more than one tile
    # nothing to compute: nothing is launched, nothing is dereferenced
    for empty in (dict(R=0), dict(C=0), dict(R=0, C=0, M=0)):
        assert fwd(logits=None, rows=None, labels=None, valid=None, ws=None, tc=None, fs=None, counts=None, shape=shape(**empty)) == 0
        assert bwd(logits=None, tc=None, gs=None, gl=None, shape=shape(**empty)) == 0
    # the workspace: host arithmetic
    ws = lambda code=0, **kw: lib.labelloss_workspace_bytes(code, shape(**kw))      # noqa: E731
    assert ws() == 0 and ws(R=rows_per_tile) == 0 and ws(R=0) == 0
    assert ws(R=rows_per_tile + 1) == 256 and ws(1, R=rows_per_tile + 1) == 256 and ws(R=9 * rows_per_tile) % 256 == 0
    assert ws(R=9 * rows_per_tile) >= 9 * 24 and ws(R=3, C=2 * _labelloss.tile()) == 256          # a long row is one tile
    assert ws(9) == -1 and b"dtype" in err() and ws(R=-1) == -1 and lib.labelloss_workspace_bytes(0, None) == -1


# ---- oracle ----------------------------------------------------------------------------------------------------------

def test_fixtures_cover_the_cases():
    assert FIXTURES == ["labelloss_devis", "labelloss_devis_matched", "labelloss_devis_none", "labelloss_image"]
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 32 << 10
        d = load_fixture(name)
        assert d["logits"].dtype == F64 and float(d["margin"]) > 1e-2 and d["target_classes"].dtype == torch.int64
    d = load_fixture("labelloss_devis")
    assert d["dims"].tolist() == [3, 7, 5, 2] and tuple(d["logits"].shape) == (1, 21, 5) and int(d["index_valid"].sum()) == 5
    assert 0.0 < float(d["class_error"]) < 100.0
    none = load_fixture("labelloss_devis_none")
    assert not bool(none["index_valid"].any()) and float(none["class_error"]) == 100.0 and bool((none["target_classes"] == 5).all())
    matched, source = load_fixture("labelloss_devis_matched"), {k: torch.from_numpy(v) for k, v in golden("boxmatch_devis_mean").items()}
    for key in ("logits", "labels", "valid", "index_i", "index_j", "index_valid"):       # the matcher fixture's inputs and matching
        assert torch.equal(matched[key], source[key]), key
    image = load_fixture("labelloss_image")
    assert image["dims"].tolist() == [2, 7, 5] and image["sizes"].tolist() == [3, 2] and 0.0 < float(image["class_error"]) < 100.0


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_equals_the_reference(name):
    d = load_fixture(name)
    logits, rows, labels, valid = fixture_operands(d)
    focal_sum, counts, classes, grad = labelloss_oracle.label_loss_terms(logits, rows, labels, valid, alpha=float(d["alpha"]),
                                                                         grad_sum=1.0 / float(d["num_boxes"]))
    assert focal_sum.dtype == F64 and counts.dtype == classes.dtype == torch.int32
    assert close(focal_sum / float(d["num_boxes"]), d["loss_ce"]) and close(grad, d["grad_logits"])
    assert torch.equal(classes.long(), d["target_classes"]) and counts[2:].tolist() == [0, 0]
    assert int(counts[0]) == (int(valid.sum()) if valid is not None else rows.numel())
    losses = labelloss_oracle.label_losses(logits, rows, labels, valid, float(d["num_boxes"]), alpha=float(d["alpha"]))
    assert close(losses["loss_ce"], d["loss_ce"]) and close(losses["class_error"], d["class_error"])


def test_oracle_rules_duplicates_background_label_and_bad_matches():
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(1, 4, 3, generator=g, dtype=F64)
    logits[0, 1] = torch.tensor([0.5, 2.0, 2.0])                 # a tie: the lowest index, 1, wins
    rows, labels = torch.tensor([1, 2, 1, 9, 0, 3]), torch.tensor([2, 3, 1, 0, 4, -1])
    valid = torch.tensor([True, True, True, True, True, False])
    focal_sum, counts, classes = labelloss_oracle.label_loss_terms(logits, rows, labels, valid)
    assert classes.tolist() == [[3, 1, 3, 3]]                    # row 1: the later match; row 2: "no object"; row 0: a bad label
    assert counts.tolist() == [3, 1, 1, 1]                       # matches 0, 1, 2 are good; only (row 1, label 1) is right
    plain = labelloss_oracle.label_loss_terms(logits, torch.tensor([1]), torch.tensor([1]))
    assert float(plain[0]) == float(focal_sum) and plain[1].tolist() == [1, 1, 0, 0]
    logits[0, 1, 0] = float("nan")
    assert labelloss_oracle.label_loss_terms(logits, rows, labels, valid)[1].tolist() == [3, 0, 1, 1]
    x = torch.tensor([[[float("inf"), -float("inf"), 30.0]]], dtype=F64)
    for label, want in ((0, [0.0, 0.0]), (1, [float("inf"), float("inf")]), (3, [float("inf"), 0.0])):
        focal, _ = labelloss_oracle.elements(x[0], torch.arange(3)[None] == label, 0.25)
        assert focal[0, :2].tolist() == want and bool(torch.isfinite(focal[0, 2]))


# ---- host ------------------------------------------------------------------------------------------------------------

def test_operators_raise_on_cpu_tensors_and_on_bad_arguments_before_any_launch(monkeypatch):
    import devis_amd
    from devis_amd import _labelloss
    from devis_amd.functions import label_loss as Y

    def no_launch(*a, **k):
        raise AssertionError("a kernel call was made")

    for name in ("forward", "backward"):
        monkeypatch.setattr(_labelloss, name, no_launch)
    logits, rows, labels = torch.zeros(1, 21, 5), torch.zeros(6, dtype=torch.int64), torch.zeros(6, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.label_loss_terms(logits, rows, labels)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.label_losses(logits, rows, labels, torch.ones(6, dtype=torch.bool), 2.0)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        Y._backward(torch.ones(()), logits, torch.zeros(1, 21, dtype=torch.int32), 0.25)
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        devis_amd.label_loss_terms(torch.zeros(1, 21, 5, dtype=torch.complex64).requires_grad_(True), rows, labels)
    for name in ("label_loss_terms", "label_losses", "patch_label_loss", "unpatch_label_loss"):
        assert name in devis_amd.__all__ and getattr(devis_amd, name) is getattr(
            devis_amd.ops if "patch" not in name else devis_amd.argument_builders, name)
    assert "no CPU path" in Y.__doc__

    meta = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="meta")      # noqa: E731
    i64 = torch.int64
    ok = (meta(2, 7, 5), meta(5, dtype=i64), meta(5, dtype=i64), meta(5, dtype=torch.bool))
    assert Y.check_labels(*ok) == (2, 7, 5, 5) and Y.check_labels(*ok[:3], None) == (2, 7, 5, 5)
    assert Y.check_labels(meta(2, 7, 5, dtype=torch.bfloat16), ok[1], ok[2], meta(5, dtype=torch.uint8)) == (2, 7, 5, 5)
    assert Y.check_labels(meta(0, 7, 5), meta(0, dtype=i64), meta(0, dtype=i64), None) == (0, 7, 5, 0)
    bad = [
        ("logits must be \\[B, N, C\\]", lambda: Y.check_labels(meta(14, 5), *ok[1:])),
        ("unsupported dtype", lambda: Y.check_labels(meta(2, 7, 5, dtype=torch.int32), *ok[1:])),
        ("rows must be int64 \\[M\\]", lambda: Y.check_labels(ok[0], meta(5, dtype=torch.int32), *ok[2:])),
        ("rows must be int64 \\[M\\]", lambda: Y.check_labels(ok[0], meta(5, 1, dtype=i64), *ok[2:])),
        ("labels must be int64 \\[M\\]", lambda: Y.check_labels(ok[0], ok[1], meta(5), ok[3])),
        ("labels has 4 matches, rows 5", lambda: Y.check_labels(ok[0], ok[1], meta(4, dtype=i64), ok[3])),
        ("valid must be bool or uint8 \\[M\\]", lambda: Y.check_labels(*ok[:3], meta(5, dtype=i64))),
        ("valid has 6 matches, rows 5", lambda: Y.check_labels(*ok[:3], meta(6, dtype=torch.bool))),
    ]
    for match, call in bad:
        with pytest.raises(RuntimeError, match=match):
            call()


def test_no_backward_call_when_logits_need_no_gradient():
    from devis_amd import ops
    from devis_amd.functions import label_loss as Y
    seen = []
    logits, classes, g = torch.zeros(1, 3, 2), torch.zeros(1, 3, dtype=torch.int32), torch.ones(())
    host = lambda *a: seen.append("host") or torch.zeros(1, 3, 2)      # noqa: E731
    op = lambda *a: seen.append("op") or torch.zeros(1, 3, 2)      # noqa: E731
    # the one formula, run the way the eager Function runs it and the way the op's register_autograd does
    assert Y.LabelLossTermsFunction.setup_context is Y.setup_context is ops.label_loss_terms_op._setup_context_fn
    assert ops.label_loss_terms_op._backward_fn.func is Y.backward
    for needs in ((False,) * 5, (True,) + (False,) * 4):
        ctx = types.SimpleNamespace(saved_tensors=(logits, classes), needs_input_grad=needs, alpha=0.25)
        before = len(seen)
        for res in (Y.backward(host, ctx, g, None, None), Y.backward(op, ctx, g, None, None)):
            assert len(res) == 5 and all(r is None for r in res[1:]) and (res[0] is None) == (not needs[0])
        assert seen[before:] == (["host", "op"] if needs[0] else [])


# ---- the drop-in of patch_label_loss ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_loss_labels_focal_gives_the_reference_losses_for_two_and_three_tuples(name, monkeypatch):
    from devis_amd import argument_builders, ops
    d = load_fixture(name)
    seen = []

    def oracle(logits, rows, labels, valid, num_boxes, **k):
        seen.append((rows, labels, valid, num_boxes, k))
        return labelloss_oracle.label_losses(logits, rows, labels, valid, num_boxes, **k)

    monkeypatch.setattr(ops, "label_losses", oracle)
    outputs, targets, indices, num_boxes = fixture_call(d)
    x = outputs["pred_logits"].clone().requires_grad_(True)
    out = argument_builders.loss_labels_focal(StandInLabelCriterion(), {"pred_logits": x}, targets, indices, num_boxes)
    assert sorted(out) == ["class_error", "loss_ce"]
    assert close(out["loss_ce"].detach(), d["loss_ce"]) and close(out["class_error"], d["class_error"])
    grad, = torch.autograd.grad(out["loss_ce"], x)
    assert close(grad, d["grad_logits"])
    (rows, labels, valid, n, k), = seen
    want = fixture_operands(d)
    assert rows.dtype == labels.dtype == torch.int64 and torch.equal(rows, want[1]) and torch.equal(labels, want[2])
    assert (valid is None) == (want[3] is None) and (valid is None or (valid.dtype == torch.bool and torch.equal(valid, want[3])))
    assert n == num_boxes and k == {"alpha": 0.25, "log": True}
    only = argument_builders.loss_labels_focal(StandInLabelCriterion(), outputs, targets, indices, num_boxes, log=False)
    assert sorted(only) == ["loss_ce"] and seen[-1][-1] == {"alpha": 0.25, "log": False}


def test_patch_label_loss_sets_and_restores_the_method_and_leaves_the_other_patches_alone():
    import devis_amd
    crit, match = label_modules()
    crit.SetCriterion.loss_masks = lambda self, *a: "their masks"
    names = ("loss_labels_focal", "loss_boxes", "loss_masks", "forward")
    current = lambda: tuple(getattr(crit.SetCriterion, n) for n in names) + (      # noqa: E731
        match.DeVISHungarianMatcher.forward, match.HungarianMatcher.forward)
    theirs = current()
    existing = crit.SetCriterion()
    previous = devis_amd.patch_label_loss(crit)
    assert previous is theirs[0] and crit.SetCriterion.loss_labels_focal is devis_amd.argument_builders.loss_labels_focal
    assert existing.loss_labels_focal.__func__ is devis_amd.argument_builders.loss_labels_focal       # criteria that exist follow
    assert current()[1:] == theirs[1:]
    undo_crit = devis_amd.patch_criterion(crit, match)               # independent of the other patches, in either order
    assert undo_crit == {"loss_boxes": theirs[1], "devis_forward": theirs[4], "image_forward": theirs[5]}
    undo_masks = devis_amd.patch_mask_losses(crit)
    devis_amd.unpatch_label_loss(crit, previous)
    assert crit.SetCriterion.loss_labels_focal is theirs[0] and crit.SetCriterion.loss_boxes is devis_amd.argument_builders.loss_boxes
    assert crit.SetCriterion.loss_masks is devis_amd.argument_builders.loss_masks
    previous = devis_amd.patch_label_loss(crit)
    devis_amd.unpatch_criterion(crit, match, undo_crit)
    devis_amd.unpatch_mask_losses(crit, undo_masks)
    assert crit.SetCriterion.loss_labels_focal is devis_amd.argument_builders.loss_labels_focal and current()[1:] == theirs[1:]
    devis_amd.unpatch_label_loss(crit, previous)
    assert current() == theirs and existing.loss_labels_focal(None, None, None, None) == "theirs"
    undo_crit = devis_amd.patch_criterion(crit, match, batch_aux=True, gpu_assignment=True)
    assert sorted(undo_crit) == ["criterion_forward", "devis_forward", "image_forward", "loss_boxes"]
    devis_amd.unpatch_criterion(crit, match, undo_crit)
    assert current() == theirs
    with pytest.raises(AttributeError):
        devis_amd.patch_label_loss(types.SimpleNamespace())


# ---- fake-tensor paths -----------------------------------------------------------------------------------------------

def _nodes(graph, name):
    return [n for n in graph.nodes if n.op == "call_function" and name in str(n.target) and "backward" not in str(n.target)]


def test_make_fx_with_fake_tensors_gives_one_op_node():
    from torch.fx.experimental.proxy_tensor import make_fx
    from devis_amd import ops
    meta = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")      # noqa: E731
    i64 = torch.int64
    for dtype, acc in ((torch.float32, torch.float32), (torch.bfloat16, torch.float32), (torch.float16, torch.float32), (F64, F64)):
        for valid in (meta(6, dtype=torch.bool), None):
            fn = ((lambda x, r, l: ops.label_loss_terms_op(x, r, l, None, 0.25)) if valid is None
                  else (lambda x, r, l, v: ops.label_loss_terms_op(x, r, l, v, 0.25)))
            args = (meta(2, 21, 5, dtype=dtype), meta(6, dtype=i64), meta(6, dtype=i64)) + (() if valid is None else (valid,))
            gm = make_fx(fn, tracing_mode="fake")(*args)
            node, = _nodes(gm.graph, "label_loss_terms")
            focal_sum, counts, classes = node.meta["val"]
            assert tuple(focal_sum.shape) == () and focal_sum.dtype == acc
            assert tuple(counts.shape) == (4,) and counts.dtype == torch.int32
            assert tuple(classes.shape) == (2, 21) and classes.dtype == torch.int32
    with pytest.raises(Exception, match="labels has 5 matches, rows 6"):
        make_fx(lambda x, r, l: ops.label_loss_terms_op(x, r, l, None, 0.25), tracing_mode="fake")(
            meta(2, 21, 5), meta(6, dtype=i64), meta(5, dtype=i64))


@pytest.mark.parametrize("dynamic", [False, True])
def test_export_gives_one_op_node_for_static_and_dynamic_sizes(dynamic):
    import devis_amd

    class Loss(torch.nn.Module):
        def forward(self, logits, rows, labels, valid):
            out = devis_amd.label_losses(logits, rows, labels, valid, 3.0)
            return out["loss_ce"], out["class_error"]

    args = (torch.empty(2, 21, 5, device="meta"), torch.empty(6, dtype=torch.int64, device="meta"),
            torch.empty(6, dtype=torch.int64, device="meta"), torch.empty(6, dtype=torch.bool, device="meta"))
    shapes = ({1: torch.export.Dim("N", min=2, max=4096)}, None, None, None) if dynamic else None
    node, = _nodes(torch.export.export(Loss(), args, dynamic_shapes=shapes).graph, "label_loss_terms")
    focal_sum, counts, classes = node.meta["val"]
    assert tuple(focal_sum.shape) == () and focal_sum.dtype == torch.float32 and tuple(counts.shape) == (4,)
    assert classes.dtype == torch.int32 and len(classes.shape) == 2 and classes.shape[0] == 2
    assert not isinstance(classes.shape[1], int) if dynamic else tuple(classes.shape) == (2, 21)


# ---- documents -------------------------------------------------------------------------------------------------------

def test_the_documents_describe_the_operator():
    read = lambda name: open(os.path.join(ROOT, name)).read()      # noqa: E731
    design, integration, readme = read("DESIGN.md"), read("INTEGRATION.md"), read("README.md")
    assert re.search(r"^## 17\. .*label loss", design, re.M | re.I)
    assert re.search(r"^#+ Criterion: label loss", integration, re.M) and "counts[2:]" in integration
    assert "patch_label_loss" in integration and "label_losses" in readme and "labelloss.h" in readme
    for text in (design, readme):
        assert "the label loss and the weighting stay on torch" not in text
    assert os.path.exists(os.path.join(ROOT, "profiles", "labelloss_resource_usage.txt"))
    assert os.path.exists(os.path.join(ROOT, "scripts", "labelloss_bench.py"))
