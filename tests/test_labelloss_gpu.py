"""GPU tests of the criterion's label loss (include/labelloss.h) against the reference fixtures and the float64 oracle of
tests/labelloss_oracle.py, run on exactly the values the operator received (16-bit logits are rounded once, before both sides
see them).

Tolerance: focal_sum within 1e-4 * max(1, |want|), the project's parity bound as tests/test_boxmatch_gpu.py states it, and
grad_logits within 1e-4 * max|want| per tensor; 1e-10 for float64; a 16-bit grad_logits may differ by one more rounding of its
storage type: eps / 2 * |want|, or half the type's smallest subnormal where the value lies below its normal range (a
float16 cannot hold less than 2^-24; a gradient of 3e-14 is stored as 0).  counts and target_classes are compared with ==."""
import pytest
import torch

import labelloss_oracle
from test_boxmatch_cpu import devis_call
from test_boxmatch_cpu import load_fixture as load_match_fixture
from test_boxmatch_gpu import count_syncs, gpu_targets
from test_labelloss_cpu import FIXTURES, StandInLabelCriterion, fixture_call, fixture_operands, label_modules, load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16]
F64 = torch.float64
# (B, N, C, M); "tile" / "tile+row": R * C is exactly one forward tile, and one row more (two tiles)
SHAPES = [(1, 21, 5, 6), (2, 7, 5, 5), (1, 1, 1, 1), (1, 3, 130, 2), (2, 300, 91, 20), "tile", "tile+row"]
GRAD_SUM = 0.5
ALPHA = 0.25


def shape_of(shape):
    if isinstance(shape, tuple):
        return shape
    from devis_amd import _labelloss
    C = 64
    assert _labelloss.tile() % C == 0
    return (1, _labelloss.tile() // C + (1 if shape == "tile+row" else 0), C, 9)


def tol_of(dtype):
    return 1e-10 if dtype == F64 else 1e-4


def rounding_of(dtype):
    """(relative, absolute) error of one rounding to a 16-bit storage type: half an ulp, of a normal value and of a subnormal."""
    if dtype not in (torch.bfloat16, torch.float16):
        return 0.0, 0.0
    info = torch.finfo(dtype)
    return info.eps / 2, info.smallest_normal * info.eps / 2


def assert_value(got, want, tol, what):
    got, want = float(got), float(want)
    print("%s: %.9g against %.9g, error %.3e" % (what, got, want, abs(got - want)))
    assert abs(got - want) <= tol * max(1.0, abs(want)), (what, got, want)


def assert_grad(got, want, tol, what, rounding=(0.0, 0.0)):
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape, what
    err = (got - want).abs()
    bound = tol * float(want.abs().max()) + (rounding[0] * want.abs()).clamp(min=rounding[1])
    print("%s: max error %.3e, max |want| %.3e" % (what, float(err.max()) if err.numel() else 0.0, float(want.abs().max()) if err.numel() else 0.0))
    assert not bool(torch.isnan(got).any()) and bool((err <= bound).all()), (what, float(err.max()))


_CASES = {}


def case(shape, dtype):
    """((logits rounded once to `dtype`, rows, labels, valid), the float64 oracle's results with the gradient) of a shape:
    computed once, shared, read only.  The rows are distinct; about a quarter of the matches is invalid; half of the others
    are made right."""
    key = (shape, dtype)
    if key not in _CASES:
        B, N, C, M = shape_of(shape)
        g = torch.Generator().manual_seed(B + 10 * N + 100 * C + M)
        logits = 3 * torch.randn(B, N, C, generator=g, dtype=F64)
        rows = torch.randperm(B * N, generator=g)[:M]
        labels = torch.randint(0, C, (M,), generator=g)
        valid = torch.rand(M, generator=g) > 0.25
        for m in range(0, M, 2):
            logits.view(-1, C)[int(rows[m]), int(labels[m])] += 8.0
        logits = logits.to(dtype)
        want = labelloss_oracle.label_loss_terms(logits.double(), rows, labels, valid, alpha=ALPHA, grad_sum=GRAD_SUM)
        _CASES[key] = ((logits, rows, labels, valid), want)
    return _CASES[key]


def on_gpu(ops):
    return tuple(None if t is None else t.to(DEV) for t in ops)


def run_op(logits, rows, labels, valid, alpha=ALPHA, grad_sum=GRAD_SUM):
    """(focal_sum, counts, target_classes, grad_logits) of the operator on the GPU."""
    import devis_amd
    x = logits.to(DEV).detach().requires_grad_(True)
    focal_sum, counts, classes = devis_amd.label_loss_terms(x, *on_gpu((rows, labels, valid)), alpha=alpha)
    assert not counts.requires_grad and not classes.requires_grad
    grad, = torch.autograd.grad(focal_sum, x, torch.tensor(grad_sum, dtype=focal_sum.dtype, device=DEV))
    return focal_sum.detach(), counts, classes, grad


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---- part 1: numerics ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_forward_and_backward_equal_the_oracle(shape, dtype):
    from devis_amd import _labelloss, _native
    ops, want = case(shape, dtype)
    B, N, C, M = shape_of(shape)
    focal_sum, counts, classes, grad = run_op(*ops)
    arith = F64 if dtype == F64 else torch.float32
    assert focal_sum.dtype == arith and tuple(focal_sum.shape) == () and grad.dtype == dtype and tuple(grad.shape) == (B, N, C)
    assert counts.dtype == classes.dtype == torch.int32 and tuple(counts.shape) == (4,) and tuple(classes.shape) == (B, N)
    assert_value(focal_sum, want[0], tol_of(dtype), "focal_sum")
    assert counts.tolist() == want[1].tolist() and torch.equal(classes.cpu(), want[2])
    assert_grad(grad, want[3], tol_of(dtype), "grad_logits", rounding_of(dtype))
    if isinstance(shape, str):          # the threshold between one launch and two lies where the test puts it
        nbytes = _labelloss.workspace_bytes(_native.dtype_code(dtype), _labelloss.Shape(B * N, C, M))
        assert (nbytes == 0) == (shape == "tile") and B * N * C == _labelloss.tile() + (C if shape == "tile+row" else 0)


@pytest.mark.parametrize("name", FIXTURES)
def test_label_losses_equal_the_fixtures(name):
    import devis_amd
    d = load_fixture(name)
    logits, rows, labels, valid = fixture_operands(d)
    for dtype in (torch.float32, F64):
        x = logits.to(dtype).to(DEV).requires_grad_(True)
        out = devis_amd.label_losses(x, *on_gpu((rows, labels, valid)), float(d["num_boxes"]), alpha=float(d["alpha"]))
        grad, = torch.autograd.grad(out["loss_ce"], x)
        assert out["loss_ce"].dtype == dtype and out["class_error"].is_cuda and tuple(out["class_error"].shape) == ()
        assert_value(out["loss_ce"].detach(), d["loss_ce"], tol_of(dtype), name + " loss_ce")
        assert_value(out["class_error"], d["class_error"], tol_of(dtype), name + " class_error")
        assert_grad(grad, d["grad_logits"], tol_of(dtype), name + " grad_logits")
        classes = devis_amd.label_loss_terms(x.detach(), *on_gpu((rows, labels, valid)))[2]
        assert torch.equal(classes.cpu().long(), d["target_classes"])
    assert sorted(devis_amd.label_losses(x.detach(), *on_gpu((rows, labels, valid)), 2.0, log=False)) == ["loss_ce"]


# ---- part 2: the rules ---------------------------------------------------------------------------------------------------

def test_duplicate_rows_the_background_label_and_invalid_matches():
    (logits, _, _, _), _ = case(SHAPES[0], torch.float32)
    C = logits.shape[-1]
    logits = logits.clone()
    logits[0, 4] = torch.tensor([0.0, 1.0, 3.0, 3.0, -1.0])          # a tie between classes 2 and 3: the lowest wins
    rows = torch.tensor([4, 9, 4, 11, 4, 9, 2])
    labels = torch.tensor([2, 1, 0, C, 3, 1, 4])
    valid = torch.tensor([True, True, True, True, True, True, False])
    got = run_op(logits, rows, labels, valid)
    want = labelloss_oracle.label_loss_terms(logits.double(), rows, labels, valid, alpha=ALPHA, grad_sum=GRAD_SUM)
    classes = got[2].cpu()
    assert int(classes[0, 4]) == 3 and int(classes[0, 9]) == 1 and int(classes[0, 11]) == C        # the highest m wins
    assert int(classes[0, 2]) == C                                                                 # an invalid match: ignored
    assert torch.equal(classes, want[2]) and got[1].tolist() == want[1].tolist()
    # six good matches, every duplicate counted against its own label: (4, 2) is right -- the tie goes to class 2 -- and
    # (4, 3), (4, 0) are not; (9, 1) twice as the row's argmax says; the label C never
    right_9 = int(logits[0, 9].argmax()) == 1
    assert got[1].tolist() == [6, 1 + 2 * int(right_9), 0, 0]
    assert_value(got[0], want[0], 1e-4, "focal_sum with duplicates")
    assert_grad(got[3], want[3], 1e-4, "grad_logits with duplicates")
    # the row of the label C is all-negative: the same as no match at all for it
    without = run_op(logits, rows[[0, 1, 2, 4, 5]], labels[[0, 1, 2, 4, 5]], None)
    assert torch.equal(without[0], got[0]) and torch.equal(without[3], got[3]) and torch.equal(without[2], got[2])
    assert without[1].tolist() == [5, got[1].tolist()[1], 0, 0]


def test_rows_and_labels_out_of_range_are_counted_and_otherwise_without_effect():
    ops, _ = case(SHAPES[4], torch.float32)
    logits, rows, labels, valid = ops
    B, N, C, M = SHAPES[4]
    clean = run_op(*ops)
    bad_rows = torch.tensor([-1, B * N, 1 << 40, -(1 << 40)])
    bad_labels = torch.tensor([-1, C + 1, 1 << 40])
    free = [r for r in range(B * N) if r not in set(rows.tolist())][:3]
    rows2 = torch.cat([bad_rows, rows, torch.tensor(free)])
    labels2 = torch.cat([torch.zeros(4, dtype=torch.int64), labels, bad_labels])
    valid2 = torch.cat([torch.tensor([True, True, True, False]), valid, torch.tensor([True, True, False])])
    got = run_op(logits, rows2, labels2, valid2)
    assert got[1].tolist() == clean[1].tolist()[:2] + [3, 2]
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2]) and torch.equal(got[3], clean[3])


def test_no_matches_and_all_invalid_matches_make_every_row_background():
    import devis_amd
    ops, _ = case(SHAPES[1], torch.float32)
    logits, rows, labels, _ = ops
    B, N, C, M = SHAPES[1]
    empty = torch.zeros(0, dtype=torch.int64)
    none = run_op(logits, empty, empty, None)
    invalid = run_op(logits, rows, labels, torch.zeros(M, dtype=torch.bool))
    as_bytes = run_op(logits, rows, labels, torch.zeros(M, dtype=torch.uint8))
    want = labelloss_oracle.label_loss_terms(logits.double(), empty, empty, alpha=ALPHA, grad_sum=GRAD_SUM)
    for got in (none, invalid, as_bytes):
        assert got[1].tolist() == [0, 0, 0, 0] and bool((got[2] == C).all()) and same(got, none)
    assert_value(none[0], want[0], 1e-4, "focal_sum of the background")
    assert_grad(none[3], want[3], 1e-4, "grad_logits of the background")
    for args in ((empty, empty, None), (rows, labels, torch.zeros(M, dtype=torch.bool))):
        out = devis_amd.label_losses(logits.to(DEV), *on_gpu(args), 2.0)
        assert float(out["class_error"]) == 100.0


def test_valid_none_equals_an_all_true_mask():
    for shape in (SHAPES[0], SHAPES[4]):
        logits, rows, labels, _ = case(shape, torch.float32)[0]
        a = run_op(logits, rows, labels, None)
        assert same(a, run_op(logits, rows, labels, torch.ones(rows.shape[0], dtype=torch.bool)))
        assert same(a, run_op(logits, rows, labels, torch.full((rows.shape[0],), 7, dtype=torch.uint8)))        # nonzero is valid


# ---- part 3: reproducibility -----------------------------------------------------------------------------------------------

def test_two_runs_a_permutation_a_batch_element_alone_and_views_give_the_same_bits():
    for dtype in (torch.float32, torch.bfloat16):
        ops, _ = case(SHAPES[4], dtype)
        logits, rows, labels, valid = ops
        B, N, C, M = SHAPES[4]
        full = run_op(*ops)
        assert same(full, run_op(*ops))                                                                 # run to run
        perm = torch.randperm(M, generator=torch.Generator().manual_seed(1))
        assert same(full, run_op(logits, rows[perm], labels[perm], valid[perm]))                        # the order of the matches
        for b in range(B):                                                                              # an element alone
            mine = (rows >= b * N) & (rows < (b + 1) * N)
            alone = run_op(logits[b:b + 1], rows[mine] - b * N, labels[mine], valid[mine])
            assert torch.equal(alone[3][0], full[3][b]) and torch.equal(alone[2][0], full[2][b])
        wide = torch.zeros(B, N + 3, 2 * C, dtype=dtype)
        wide[:, 1:N + 1, 5:5 + C] = logits
        view = wide.to(DEV)[:, 1:N + 1, 5:5 + C]
        assert not view.is_contiguous() and same(full, run_op(view, rows, labels, valid))              # a non-contiguous view
        turned = logits.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
        assert not turned.is_contiguous() and same(full, run_op(turned, rows, labels, valid))


# ---- part 4: extreme logits --------------------------------------------------------------------------------------------------

def test_extreme_logits_follow_the_formula():
    (logits, rows, labels, valid), _ = case(SHAPES[0], torch.float32)
    C = logits.shape[-1]
    at30 = logits.clone()
    at30[0, 0], at30[0, 1] = 30.0, -30.0
    at30[0, int(rows[0])] = torch.tensor([30.0, -30.0, 30.0, -30.0, 30.0])
    got = run_op(at30, rows, labels, valid)
    want = labelloss_oracle.label_loss_terms(at30.double(), rows, labels, valid, alpha=ALPHA, grad_sum=GRAD_SUM)
    assert_value(got[0], want[0], 1e-4, "focal_sum at +-30")
    assert_grad(got[3], want[3], 1e-4, "grad_logits at +-30")
    assert got[1].tolist() == want[1].tolist()
    # +-inf where the formula gives 0: +inf on a positive, -inf on a negative
    classes = want[2]
    r = int(rows[torch.nonzero(valid)[0]])
    pos = int(classes[0, r])
    zero = logits.clone()
    zero[0, r, pos] = float("inf")
    zero[0, r, (pos + 1) % C] = -float("inf")
    free = [q for q in range(logits.shape[1]) if int(classes[0, q]) == C][0]
    zero[0, free, 2] = -float("inf")
    got = run_op(zero, rows, labels, valid)
    want = labelloss_oracle.label_loss_terms(zero.double(), rows, labels, valid, alpha=ALPHA, grad_sum=GRAD_SUM)
    assert bool(torch.isfinite(got[0])) and torch.equal(got[2].cpu(), want[2]) and got[1].tolist() == want[1].tolist()
    assert_value(got[0], want[0], 1e-4, "focal_sum with infinite logits of no loss")
    touched = torch.zeros_like(zero, dtype=torch.bool)
    touched[0, r, pos] = touched[0, r, (pos + 1) % C] = touched[0, free, 2] = True
    assert not bool(torch.isnan(got[3].cpu()[~touched]).any())
    assert_grad(got[3].cpu()[~touched], want[3][~touched], 1e-4, "grad_logits beside infinite logits")
    # and where it gives inf: +inf on a negative, -inf on a positive
    for value, c in ((float("inf"), (pos + 1) % C), (-float("inf"), pos)):
        x = logits.clone()
        x[0, r, c] = value
        got = run_op(x, rows, labels, valid)
        assert float(got[0]) == float("inf") and torch.equal(got[2].cpu(), classes)
        others = torch.ones_like(x, dtype=torch.bool)
        others[0, r, c] = False
        assert not bool(torch.isnan(got[3].cpu()[others]).any())


def test_a_nan_logit_poisons_the_sum_its_row_and_its_own_gradient_only():
    (logits, rows, labels, valid), want = case(SHAPES[0], torch.float32)
    clean = run_op(logits, rows, labels, valid)
    m = [k for k in range(rows.shape[0]) if bool(valid[k]) and k % 2 == 0][0]           # a good match that is right
    r, c = int(rows[m]), (int(labels[m]) + 1) % logits.shape[-1]
    x = logits.clone()
    x[0, r, c] = float("nan")
    got = run_op(x, rows, labels, valid)
    assert bool(torch.isnan(got[0])) and torch.equal(got[2], clean[2])
    assert got[1].tolist() == [clean[1].tolist()[0], clean[1].tolist()[1] - 1, 0, 0]       # its row is never correct
    nan = torch.isnan(got[3]).cpu()
    assert int(nan.sum()) == 1 and bool(nan[0, r, c])
    assert torch.equal(got[3].cpu()[~nan], clean[3].cpu()[~nan])


# ---- part 5: host paths ------------------------------------------------------------------------------------------------------

def test_empty_calls_launch_nothing(monkeypatch):
    import devis_amd
    from devis_amd import _labelloss
    monkeypatch.setattr(_labelloss, "forward", lambda *a, **k: pytest.fail("a kernel call was made"))
    monkeypatch.setattr(_labelloss, "backward", lambda *a, **k: pytest.fail("a kernel call was made"))
    idx = torch.zeros(3, dtype=torch.int64, device=DEV)
    for shape in ((0, 7, 5), (2, 0, 5), (2, 7, 0)):
        x = torch.zeros(shape, device=DEV, requires_grad=True)
        focal_sum, counts, classes = devis_amd.label_loss_terms(x, idx, idx)
        assert float(focal_sum.detach()) == 0.0 and counts.tolist() == [0, 0, 0, 0] and tuple(classes.shape) == shape[:2]
        grad, = torch.autograd.grad(focal_sum, x)
        assert tuple(grad.shape) == shape
        assert float(devis_amd.label_losses(x, idx, idx, None, 2.0)["class_error"]) == 100.0


def stock_loss_labels_focal(logits, targets, indices, num_boxes, alpha):
    """The reference's formulation of the label loss for DeVIS triples, restated: what the operator replaces."""
    C = logits.shape[2]
    batch = torch.cat([torch.full_like(src, i)[mask] for i, (src, _, mask) in enumerate(indices)])
    src = torch.cat([src[mask] for (src, _, mask) in indices])
    wanted = torch.cat([t["labels"][J[mask]] for t, (_, J, mask) in zip(targets, indices)])
    classes = torch.full(logits.shape[:2], C, dtype=torch.int64, device=logits.device)
    classes[(batch, src)] = wanted
    onehot = torch.zeros([logits.shape[0], logits.shape[1], C + 1], dtype=logits.dtype, device=logits.device)
    onehot.scatter_(2, classes.unsqueeze(-1), 1)
    onehot = onehot[:, :, :-1]
    prob = logits.sigmoid()
    ce = torch.nn.functional.binary_cross_entropy_with_logits(logits, onehot, reduction="none")
    p_t = prob * onehot + (1 - prob) * (1 - onehot)
    loss = (alpha * onehot + (1 - alpha) * (1 - onehot)) * ce * (1 - p_t) ** 2
    return loss.mean(1).sum() / num_boxes * logits.shape[1]


def test_no_synchronising_call_with_device_indices_where_the_stock_formulation_has_one():
    import devis_amd
    d = load_fixture("labelloss_devis")
    outputs, targets, indices, num_boxes = fixture_call(d)
    logits = outputs["pred_logits"].float().to(DEV).requires_grad_(True)
    targets = gpu_targets(targets)
    indices = [tuple(t.to(DEV) for t in entry) for entry in indices]
    N = logits.shape[1]
    rows, labels, valid = indices[0][0], targets[0]["labels"][indices[0][1]], indices[0][2]

    def operator():
        out = devis_amd.label_losses(logits, rows, labels, valid, num_boxes, alpha=ALPHA)
        grad, = torch.autograd.grad(out["loss_ce"], logits)
        return out, grad

    crit, _ = label_modules()
    previous = devis_amd.patch_label_loss(crit)
    try:
        criterion = crit.SetCriterion()

        def patched():
            out = criterion.loss_labels_focal({"pred_logits": logits}, targets, indices, num_boxes)
            grad, = torch.autograd.grad(out["loss_ce"], logits)
            return out, grad

        def stock():
            loss = stock_loss_labels_focal(logits, targets, indices, num_boxes, ALPHA)
            grad, = torch.autograd.grad(loss, logits)
            return {"loss_ce": loss}, grad

        results = {}
        for name, fn in (("operator", operator), ("patched", patched), ("stock", stock)):
            fn()                                                        # (loads the library, warms the allocator)
            results[name], syncs = count_syncs(fn)
            print(name, [str(w.message) for w in syncs])
            assert (len(syncs) >= 1) if name == "stock" else (len(syncs) == 0), (name, [str(w.message) for w in syncs])
    finally:
        devis_amd.unpatch_label_loss(crit, previous)
    assert N == 21 and same(results["operator"][1:], results["patched"][1:])
    assert torch.equal(results["operator"][0]["loss_ce"], results["patched"][0]["loss_ce"])
    for name in ("operator", "stock"):
        assert_value(results[name][0]["loss_ce"].detach(), d["loss_ce"], 1e-4, name + " loss_ce")
        assert_grad(results[name][1], d["grad_logits"], 1e-4, name + " grad_logits")
    assert_value(results["patched"][0]["class_error"], d["class_error"], 1e-4, "class_error")


def test_patched_loss_labels_focal_takes_host_indices_beside_device_logits():
    import devis_amd
    crit, _ = label_modules()
    previous = devis_amd.patch_label_loss(crit)
    try:
        for name in FIXTURES:
            d = load_fixture(name)
            outputs, targets, indices, num_boxes = fixture_call(d)
            logits = outputs["pred_logits"].float().to(DEV).requires_grad_(True)
            for where in ("host", "device"):
                idx = indices if where == "host" else [tuple(t.to(DEV) for t in entry) for entry in indices]
                out = crit.SetCriterion().loss_labels_focal({"pred_logits": logits}, gpu_targets(targets), idx, num_boxes)
                grad, = torch.autograd.grad(out["loss_ce"], logits)
                assert_value(out["loss_ce"].detach(), d["loss_ce"], 1e-4, "%s %s loss_ce" % (name, where))
                assert_value(out["class_error"], d["class_error"], 1e-4, "%s %s class_error" % (name, where))
                assert_grad(grad, d["grad_logits"], 1e-4, "%s %s grad_logits" % (name, where))
    finally:
        devis_amd.unpatch_label_loss(crit, previous)
    assert crit.SetCriterion.loss_labels_focal is StandInLabelCriterion.loss_labels_focal


def test_hip_graph_replay_with_changed_inputs_equals_eager():
    import devis_amd
    from devis_amd import ops as O
    for shape in (SHAPES[0], SHAPES[4]):                    # one launch, and tiles with a combine
        first, _ = case(shape, torch.float32)
        logits, rows, labels, valid = (t.clone() for t in on_gpu(first))
        grad_sum = torch.full((), GRAD_SUM, device=DEV)

        def call():
            focal_sum, counts, classes = devis_amd.label_loss_terms(logits, rows, labels, valid, alpha=ALPHA)      # noqa: B023
            return focal_sum, counts, classes, O.label_loss_terms_backward(grad_sum, logits, classes, ALPHA)      # noqa: B023

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()          # warm up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = call()
        B, N, C, M = shape
        for k in range(2):
            g = torch.Generator().manual_seed(40 + k)
            logits.copy_((3 * torch.randn(B, N, C, generator=g)).to(DEV))
            rows.copy_(torch.randperm(B * N, generator=g)[:M].to(DEV))
            labels.copy_(torch.randint(0, C, (M,), generator=g).to(DEV))
            valid.copy_((torch.rand(M, generator=g) > 0.25).to(DEV))
            rows[k] = B * N + k                             # and a bad row: the counts are written, not added to, per replay
            graph.replay()
            torch.cuda.synchronize()
            eager = call()
            assert same(out, eager) and out[1].tolist()[2] == int(valid[k])
            want = labelloss_oracle.label_loss_terms(logits.cpu().double(), rows.cpu(), labels.cpu(), valid.cpu(), alpha=ALPHA, grad_sum=GRAD_SUM)
            assert out[1].tolist() == want[1].tolist() and torch.equal(out[2].cpu(), want[2])
            assert_value(out[0], want[0], 1e-4, "graph replay focal_sum")
            assert_grad(out[3], want[3], 1e-4, "graph replay grad_logits")


def test_compile_fullgraph_and_export_give_eagers_bits():
    import devis_amd

    def losses(x, r, l, v):
        out = devis_amd.label_losses(x, r, l, v, 3.0)
        return out["loss_ce"], out["class_error"]

    compiled = torch.compile(lambda x, r, l, v: devis_amd.label_loss_terms(x, r, l, v), fullgraph=True)
    scale = torch.full((), GRAD_SUM, device=DEV)
    for shape in (SHAPES[0], SHAPES[1], SHAPES[3]):                                     # N, C and M change
        ops = on_gpu(case(shape, torch.float32)[0])
        x = ops[0].clone().requires_grad_(True)
        want = devis_amd.label_loss_terms(x, *ops[1:])
        want_grad, = torch.autograd.grad(want[0], x, scale)
        y = ops[0].clone().requires_grad_(True)
        got = compiled(y, *ops[1:])
        grad, = torch.autograd.grad(got[0], y, scale)
        assert same(got, want) and torch.equal(grad, want_grad)

    class Loss(torch.nn.Module):
        def forward(self, x, r, l, v):
            return losses(x, r, l, v)

    ops = on_gpu(case(SHAPES[0], torch.float32)[0])
    got, want = torch.export.export(Loss(), ops).module()(*ops), losses(*ops)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- part 6: behind the matcher ----------------------------------------------------------------------------------------------

def test_matcher_then_label_loss_without_a_synchronising_call():
    import devis_amd
    d, m = load_fixture("labelloss_devis_matched"), load_match_fixture("boxmatch_devis_mean")
    crit, match = label_modules()
    undo_crit = devis_amd.patch_criterion(crit, match, gpu_assignment=True)
    undo_label = devis_amd.patch_label_loss(crit)
    try:
        outputs, targets = devis_call(m)
        logits = outputs["pred_logits"].float().to(DEV).requires_grad_(True)
        outputs = {"pred_logits": logits, "pred_boxes": outputs["pred_boxes"].float().to(DEV)}
        targets = gpu_targets(targets)
        matcher, criterion = match.DeVISHungarianMatcher(m), crit.SetCriterion()

        def step():
            indices = matcher({k: v.detach() for k, v in outputs.items()}, targets)
            out = criterion.loss_labels_focal(outputs, targets, indices, float(d["num_boxes"]))
            grad, = torch.autograd.grad(out["loss_ce"], logits)
            return out, grad, indices

        step()                                                          # (loads the library, warms the allocator)
        (out, grad, indices), syncs = count_syncs(step)
        assert len(syncs) == 0, [str(w.message) for w in syncs]
    finally:
        devis_amd.unpatch_label_loss(crit, undo_label)
        devis_amd.unpatch_criterion(crit, match, undo_crit)
    (index_i, index_j, index_valid), = indices
    assert index_i.is_cuda and torch.equal(index_i.cpu(), d["index_i"]) and torch.equal(index_valid.cpu(), d["index_valid"])
    assert_value(out["loss_ce"].detach(), d["loss_ce"], 1e-4, "loss_ce behind the matcher")
    assert_value(out["class_error"], d["class_error"], 1e-4, "class_error behind the matcher")
    assert_grad(grad, d["grad_logits"], 1e-4, "grad_logits behind the matcher")
