"""GPU tests of the criterion's matching cost and box losses (include/boxmatch.h) against the reference fixtures and the
float64 oracle of tests/boxmatch_oracle.py, run on exactly the values the operator received (16-bit inputs are rounded once,
before both sides see them).

Tolerance, per element: |got - want| <= 1e-4 * max(1, |want|), the project's parity bound, and 1e-10 * max(1, |want|) for
float64; a 16-bit grad_src may differ by one more rounding of its storage type, eps / 2 * |want|."""
import warnings

import pytest
import torch

import boxmatch_oracle
from test_boxmatch_cpu import (devis_call, devis_operands, image_call, image_operands, load_fixture, modules, same_tensors,
                               tie_cases, weights)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16]
F64 = torch.float64
SHAPES = [(1, 3, 7, 4, 5), (2, 1, 14, 5, 5), (3, 6, 50, 9, 40), (1, 1, 1, 1, 1)]        # (L, F, R, T, C)
WEIGHTS = dict(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)


def tol_of(dtype):
    return 1e-10 if dtype == F64 else 1e-4


def assert_close(got, want, tol, what, extra=0.0):
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape, what
    err = (got - want).abs()
    bound = tol * want.abs().clamp(min=1) + extra * want.abs()
    worst = float((err - bound).max()) if err.numel() else 0.0
    print("%s: max error %.3e" % (what, float(err.max()) if err.numel() else 0.0))
    assert not bool(torch.isnan(got).any()) and worst <= 0.0, (what, float(err.max()))


def boxes_of(g, *shape):
    wh = 0.05 + 0.45 * torch.rand(*shape, 2, generator=g, dtype=F64)
    return torch.cat([0.2 + 0.6 * torch.rand(*shape, 2, generator=g, dtype=F64), wh], -1)


_CASES = {}


def cost_case(shape, dtype):
    """(operands rounded once to `dtype`, the float64 oracle's cost per l1 mode) of a shape: computed once, shared, read only."""
    key = (shape, dtype)
    if key not in _CASES:
        L, Fr, R, T, C = shape
        g = torch.Generator().manual_seed(sum(shape))
        ops = ((3 * torch.randn(L, Fr, R, C, generator=g, dtype=F64)).to(dtype), boxes_of(g, L, Fr, R).to(dtype),
               torch.randint(0, C, (T, Fr), generator=g), boxes_of(g, T, Fr).to(dtype))
        want = {l1: boxmatch_oracle.match_cost(ops[0].double(), ops[1].double(), ops[2], ops[3].double(), l1=l1, **WEIGHTS)[0]
                for l1 in ("mean", "sum")}
        _CASES[key] = (ops, want)
    return _CASES[key]


def on_gpu(ops):
    return tuple(t.to(DEV) for t in ops)


def count_syncs(fn):
    """(fn's result, the warnings torch.cuda.set_sync_debug_mode("warn") raised for synchronising calls while it ran)."""
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return out, [w for w in seen if "called a synchronizing" in str(w.message)]


# ---- part 1: match_cost numerics --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_match_cost_equals_the_fixtures(dtype):
    import devis_amd
    for name in ("boxmatch_devis_mean", "boxmatch_devis_sum", "boxmatch_image"):
        d = load_fixture(name)
        image = name == "boxmatch_image"
        ops = image_operands(d) if image else devis_operands(d)
        ops = tuple(t if t.dtype == torch.int64 else t.to(dtype) for t in ops)
        l1 = "sum" if image or bool(d["use_sum"]) else "mean"
        cost, status = devis_amd.match_cost(*on_gpu(ops), l1=l1, alpha=float(d["alpha"]), **weights(d))
        assert cost.dtype == (F64 if dtype == F64 else torch.float32) and status.dtype == torch.int32 and status.tolist() == [0, 0, 0]
        if dtype in (torch.float32, F64):           # the fixture's own inputs
            if image:
                blocks = cost.reshape(2, 7, 5)
                assert_close(blocks[0, :, :3], d["cost_0"], tol_of(dtype), name + " block 0")
                assert_close(blocks[1, :, 3:], d["cost_1"], tol_of(dtype), name + " block 1")
            else:
                assert_close(cost[0], d["cost"], tol_of(dtype), name)
        want = boxmatch_oracle.match_cost(ops[0].double(), ops[1].double(), ops[2], ops[3].double(), l1=l1,
                                          alpha=float(d["alpha"]), **weights(d))[0]
        assert_close(cost, want, tol_of(dtype), name + " (oracle on the rounded inputs)")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_match_cost_equals_the_oracle(shape, dtype):
    import devis_amd
    ops, want = cost_case(shape, dtype)
    dev = on_gpu(ops)
    for l1 in ("mean", "sum"):
        cost, status = devis_amd.match_cost(*dev, l1=l1, **WEIGHTS)
        assert tuple(cost.shape) == (shape[0], shape[2], shape[3]) and status.tolist() == [0, 0, 0]
        assert_close(cost, want[l1], tol_of(dtype), "%s %s" % (shape, l1))
    if dtype in (torch.bfloat16, torch.float16):       # float32 targets beside 16-bit predictions: the same values
        wide, _ = devis_amd.match_cost(dev[0], dev[1], dev[2], dev[3].float(), l1="mean", **WEIGHTS)
        assert torch.equal(wide, devis_amd.match_cost(*dev, l1="mean", **WEIGHTS)[0])


def test_empty_problems_launch_nothing(monkeypatch):
    import devis_amd
    from devis_amd import _boxmatch
    monkeypatch.setattr(_boxmatch, "cost", lambda *a, **k: pytest.fail("a kernel call was made"))
    x = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=DEV)      # noqa: E731
    for L, T, R in ((2, 0, 7), (0, 4, 7), (2, 4, 0)):
        cost, status = devis_amd.match_cost(x(L, 3, R, 5), x(L, 3, R, 4), x(T, 3, dtype=torch.int64), x(T, 3, 4))
        assert tuple(cost.shape) == (L, R, T) and status.tolist() == [0, 0, 0] and status.dtype == torch.int32


def test_extreme_logits_give_finite_entries_and_those_at_30_follow_the_formula():
    import devis_amd
    (logits, boxes, labels, tgt), _ = cost_case(SHAPES[0], torch.float32)
    logits = logits.clone()
    logits[0, :, 0, :], logits[0, :, 1, :] = 30.0, -30.0
    want = boxmatch_oracle.match_cost(logits.double(), boxes.double(), labels, tgt.double(), **WEIGHTS)[0]
    logits[0, :, 2, :], logits[0, :, 3, :] = float("inf"), -float("inf")
    cost, _ = devis_amd.match_cost(*on_gpu((logits, boxes, labels, tgt)), **WEIGHTS)
    assert bool(torch.isfinite(cost).all())
    keep = [0, 1, 4, 5, 6]
    assert_close(cost[0, keep], want[0, keep], 1e-4, "logits of +-30")
    # at +-inf: p is exactly 1 / 0, so the class term is -(1 - alpha) * -log(1e-8) / alpha * -log(1e-8)
    rest = boxmatch_oracle.match_cost(logits.double(), boxes.double(), labels, tgt.double(), cost_class=0.0, cost_bbox=5.0, cost_giou=2.0)[0]
    assert_close(cost[0, 2] - rest[0, 2].to(DEV), torch.full((4,), -2.0 * 0.75 * 18.420680743952367, dtype=F64), 1e-4, "+inf")
    assert_close(cost[0, 3] - rest[0, 3].to(DEV), torch.full((4,), 2.0 * 0.25 * 18.420680743952367, dtype=F64), 1e-4, "-inf")


def test_nan_inputs_give_nan_exactly_in_the_entries_that_read_them():
    import devis_amd
    (logits, boxes, labels, tgt), _ = cost_case(SHAPES[0], torch.float32)
    clean = devis_amd.match_cost(*on_gpu((logits, boxes, labels, tgt)), **WEIGHTS)[0]
    logits, boxes, tgt = logits.clone(), boxes.clone(), tgt.clone()
    logits[0, 1, 2, int(labels[3, 1])] = float("nan")           # read by the entries (r = 2, t) with labels[t, 1] equal to it
    boxes[0, 2, 5, 1] = float("nan")                            # read by row 5
    tgt[1, 0, 3] = float("nan")                                 # read by target 1
    cost, status = devis_amd.match_cost(*on_gpu((logits, boxes, labels, tgt)), **WEIGHTS)
    want = torch.zeros(7, 4, dtype=torch.bool)
    want[2] = labels[:, 1] == labels[3, 1]
    want[5], want[:, 1] = True, True
    assert torch.equal(torch.isnan(cost[0]).cpu(), want) and status.tolist() == [0, 0, 0]
    assert torch.equal(cost[0][~want.to(DEV)], clean[0][~want.to(DEV)])


def test_an_entry_has_the_same_bits_alone_and_in_a_larger_call():
    import devis_amd
    for dtype in (torch.float32, torch.bfloat16):
        logits, boxes, labels, tgt = on_gpu(cost_case(SHAPES[2], dtype)[0])
        full = devis_amd.match_cost(logits, boxes, labels, tgt, **WEIGHTS)[0]
        one = devis_amd.match_cost(logits[1:2], boxes[1:2], labels, tgt, **WEIGHTS)[0]             # a view at an offset
        assert torch.equal(one[0], full[1])
        some = devis_amd.match_cost(logits, boxes, labels[[7, 2, 4]], tgt[[7, 2, 4]], **WEIGHTS)[0]
        assert torch.equal(some, full[:, :, [7, 2, 4]])
        rows = devis_amd.match_cost(logits[:, :, 10:33], boxes[:, :, 10:33], labels, tgt, **WEIGHTS)[0]       # a non-dense view
        assert torch.equal(rows, full[:, 10:33])
        assert torch.equal(full, devis_amd.match_cost(logits, boxes, labels, tgt, **WEIGHTS)[0])                # and run to run


def test_status_counts_degenerate_boxes_and_bad_labels_and_the_patched_matcher_raises(monkeypatch):
    import devis_amd
    (logits, boxes, labels, tgt), _ = cost_case(SHAPES[0], torch.float32)
    bad_tgt = tgt.clone()
    bad_tgt[2, 1, 2] = -0.1
    cost, status = devis_amd.match_cost(*on_gpu((logits, boxes, labels, bad_tgt)), **WEIGHTS)
    assert status.tolist() == [0, 1, 0]
    bad_boxes = boxes.clone()
    bad_boxes[0, 0, 3, 3], bad_boxes[0, 2, 6, 2] = -0.2, -0.3
    assert devis_amd.match_cost(*on_gpu((logits, bad_boxes, labels, tgt)), **WEIGHTS)[1].tolist() == [2, 0, 0]
    # a label equal to C, for a frame whose rows are not the last of the logits tensor: even an unguarded read of
    # logits[0, 0, r, C] would be logits[0, 0, r + 1, 0], inside the tensor
    bad_labels = labels.clone()
    bad_labels[1, 0] = 5
    cost, status = devis_amd.match_cost(*on_gpu((logits, boxes, bad_labels, tgt)), **WEIGHTS)
    assert status.tolist() == [0, 0, 1]
    assert bool(torch.isnan(cost[0, :, 1]).all()) and bool(torch.isfinite(cost[0][:, [0, 2, 3]]).all())

    d = load_fixture("boxmatch_devis_mean")
    crit, match = modules()
    previous = devis_amd.patch_criterion(crit, match)
    try:
        outputs, targets = devis_call(d)
        outputs = {k: v.float().to(DEV) for k, v in outputs.items()}
        gpu = lambda t: {k: (v.float() if v.dtype == F64 else v).to(DEV) for k, v in t.items()}      # noqa: E731
        matcher = match.DeVISHungarianMatcher(d)
        t = gpu(targets[0])
        t["boxes"][4, 3] = -0.5
        with pytest.raises(AssertionError, match="1 target box"):
            matcher(outputs, [t])
        t = gpu(targets[0])
        t["labels"][1] = 5
        with pytest.raises(IndexError, match="outside \\[0, 5\\)"):
            matcher(outputs, [t])
    finally:
        devis_amd.unpatch_criterion(crit, match, previous)


# ---- part 2: patches, box loss, compile and capture ------------------------------------------------------------------------

def gpu_targets(targets, dtype=torch.float32):
    return [{k: (v.to(dtype) if v.is_floating_point() else v).to(DEV) for k, v in t.items()} for t in targets]


@pytest.fixture()
def patched():
    import devis_amd
    crit, match = modules()
    previous = devis_amd.patch_criterion(crit, match, batch_aux=True)
    yield crit, match
    devis_amd.unpatch_criterion(crit, match, previous)


def test_patched_matchers_return_the_fixtures_indices_with_one_synchronising_transfer(patched):
    crit, match = patched
    for name in ("boxmatch_devis_mean", "boxmatch_devis_sum"):
        d = load_fixture(name)
        outputs, targets = devis_call(d)
        outputs, targets = {k: v.float().to(DEV) for k, v in outputs.items()}, gpu_targets(targets)
        matcher = match.DeVISHungarianMatcher(d)
        matcher(outputs, targets)                                                       # (loads the library, warms the allocator)
        ((index_i, index_j, index_valid),), syncs = count_syncs(lambda: matcher(outputs, targets))      # noqa: B023
        assert len(syncs) == 1, [str(w.message) for w in syncs]
        assert index_i.device.type == index_j.device.type == "cpu" and index_valid.device == targets[0]["valid"].device
        assert same_tensors((index_i, index_j, index_valid.cpu()), (d["index_i"], d["index_j"], d["index_valid"]))
    d = load_fixture("boxmatch_image")
    outputs, targets = image_call(d)
    outputs, targets = {k: v.float().to(DEV) for k, v in outputs.items()}, gpu_targets(targets)
    out, syncs = count_syncs(lambda: match.HungarianMatcher(d)(outputs, targets))
    assert len(syncs) == 1, [str(w.message) for w in syncs]
    for b, pair in enumerate(out):
        assert same_tensors(pair, (d["index_i_%d" % b], d["index_j_%d" % b]))


@pytest.mark.parametrize("kind", ["devis", "image"])
def test_batch_aux_equals_the_per_call_route_with_one_synchronising_transfer(kind, patched):
    import devis_amd
    crit, match = patched
    d = load_fixture("boxmatch_devis_mean" if kind == "devis" else "boxmatch_image")
    top, targets = devis_call(d) if kind == "devis" else image_call(d)
    g = torch.Generator().manual_seed(3)
    layer = lambda: {"pred_logits": (top["pred_logits"] + 0.5 * torch.randn(top["pred_logits"].shape, generator=g, dtype=F64)).float().to(DEV),      # noqa: E731
                     "pred_boxes": (top["pred_boxes"] * (1 + 0.1 * torch.rand(top["pred_boxes"].shape, generator=g, dtype=F64))).float().to(DEV)}
    outputs = dict({k: v.float().to(DEV) for k, v in top.items()}, aux_outputs=[layer() for _ in range(5)])
    targets = gpu_targets(targets)
    matcher = (match.DeVISHungarianMatcher if kind == "devis" else match.HungarianMatcher)(d)
    criterion = crit.SetCriterion(matcher)
    per_call = [matcher(o, targets) for o in [{k: v for k, v in outputs.items() if k != "aux_outputs"}] + outputs["aux_outputs"]]
    batched, syncs = count_syncs(lambda: criterion.forward(outputs, targets))
    assert len(syncs) == 1, [str(w.message) for w in syncs]
    assert len(batched) == 6 and "indices" not in outputs and all("indices" not in a for a in outputs["aux_outputs"])
    for got, want in zip(batched, per_call):
        assert len(got) == len(want) and all(same_tensors(a, b) for a, b in zip(got, want))
    first = (d["index_i"], d["index_j"], d["index_valid"].to(DEV)) if kind == "devis" else (d["index_i_0"], d["index_j_0"])
    assert same_tensors(batched[0][0], first)


def box_case(N, dtype, seed=0):
    """(src, target) [N, 4] rounded once to `dtype`; the first rows are the tie cases (identical boxes first)."""
    g = torch.Generator().manual_seed(seed + N)
    src, tgt = boxes_of(g, N), boxes_of(g, N)
    ts, tt = tie_cases()
    k = min(N, ts.shape[0])
    src[:k], tgt[:k] = ts[:k], tt[:k]
    src, tgt = src.to(dtype), tgt.to(dtype)
    if N:
        tgt[0] = src[0]
    return src, tgt


def run_box_op(src, tgt, grads):
    import devis_amd
    s = src.to(DEV).requires_grad_(True)
    l1, giou = devis_amd.box_loss_terms(s, tgt.to(DEV))
    gs, = torch.autograd.grad([l1, giou], s, [g.to(DEV, l1.dtype) for g in grads])
    return l1.detach(), giou.detach(), gs


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("N", [0, 1, 9, 300])
def test_box_loss_terms_forward_and_backward_equal_the_oracle(N, dtype):
    arith = F64 if dtype == F64 else torch.float32
    src, tgt = box_case(N, dtype)
    g = torch.Generator().manual_seed(1)
    grads = (torch.randn(N, generator=g, dtype=F64).to(arith), torch.randn(N, generator=g, dtype=F64).to(arith))
    l1, giou, gs = run_box_op(src, tgt, grads)
    assert l1.dtype == giou.dtype == arith and gs.dtype == dtype and tuple(gs.shape) == (N, 4) and tuple(l1.shape) == (N,)
    wl, wg, wgrad = boxmatch_oracle.box_loss_terms(src.double(), tgt.double(), grads=tuple(x.double() for x in grads))
    rounding = torch.finfo(dtype).eps / 2 if dtype in (torch.bfloat16, torch.float16) else 0.0
    assert_close(l1, wl, tol_of(dtype), "l1")
    assert_close(giou, wg, tol_of(dtype), "giou")
    assert_close(gs, wgrad, tol_of(dtype), "grad_src", extra=rounding)
    again = run_box_op(src, tgt, grads)                                                    # a second run: the same bits
    assert all(torch.equal(a, b) for a, b in zip((l1, giou, gs), again))
    if N:       # the tie row against torch autograd's gradient of the restated formula, on the device's own float64
        s = src[:1].double().to(DEV).requires_grad_(True)
        t = tgt[:1].double().to(DEV)
        loss = ((s - t).abs().sum(-1) * grads[0][:1].double().to(DEV)).sum() + ((1 - boxmatch_oracle.giou(s, t)) * grads[1][:1].double().to(DEV)).sum()
        want, = torch.autograd.grad(loss, s)
        assert_close(gs[:1], want.cpu(), tol_of(dtype), "tie row", extra=rounding)
        assert float(gs[0, :2].abs().max()) == 0.0                                         # the halves cancel exactly
    if dtype in (torch.bfloat16, torch.float16) and N:                                     # float32 targets beside 16-bit boxes
        wide = run_box_op(src, tgt.float(), grads)
        assert all(torch.equal(a, b) for a, b in zip((l1, giou, gs), wide))


def test_box_losses_equal_the_fixture_and_nothing_warns_under_deterministic_algorithms():
    import devis_amd
    d = load_fixture("boxmatch_boxes")
    torch.use_deterministic_algorithms(True)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            for dtype in (torch.float32, F64):
                s = d["src"].to(dtype).to(DEV).requires_grad_(True)
                out = devis_amd.box_losses(s, d["target"].to(dtype).to(DEV), float(d["num_boxes"]))
                grad, = torch.autograd.grad(out["loss_bbox"] + out["loss_giou"], s)
                assert_close(out["loss_bbox"], d["loss_bbox"], tol_of(dtype), "loss_bbox")
                assert_close(out["loss_giou"], d["loss_giou"], tol_of(dtype), "loss_giou")
                assert_close(grad, d["grad_src"], tol_of(dtype), "grad_src")
    finally:
        torch.use_deterministic_algorithms(False)
    empty = devis_amd.box_losses(torch.zeros(0, 4, device=DEV, requires_grad=True), torch.zeros(0, 4, device=DEV), 3.0)
    assert float(empty["loss_bbox"].detach()) == 0.0 and float(empty["loss_giou"].detach()) == 0.0
    with pytest.raises(RuntimeError, match="no gradient"):
        devis_amd.box_loss_terms(d["src"].to(DEV), d["target"].to(DEV).requires_grad_(True))


def test_no_backward_launch_when_src_needs_no_gradient(monkeypatch):
    import devis_amd
    from devis_amd import _boxmatch
    src, tgt = (t.to(DEV) for t in box_case(9, torch.float32))
    scale = torch.ones((), device=DEV, requires_grad=True)
    monkeypatch.setattr(_boxmatch, "loss_backward", lambda *a, **k: pytest.fail("a backward launch was made"))
    out = devis_amd.box_losses(src, tgt, 3.0)
    assert not out["loss_bbox"].requires_grad
    l1, giou = devis_amd.box_loss_terms(src, tgt)
    ((l1 + giou).sum() * scale).backward()              # a graph whose only leaf is not src
    assert scale.grad is not None


def test_patched_loss_boxes_on_the_gpu(patched):
    crit, match = patched
    d = load_fixture("boxmatch_boxes")
    pred = d["src"].float().reshape(1, 9, 4).to(DEV).requires_grad_(True)
    targets = [{"boxes": d["target"].float().to(DEV)}]
    order = torch.arange(9)
    for indices in ([(order, order)], [(order, order, torch.ones(9, dtype=torch.bool))]):
        out = crit.SetCriterion().loss_boxes({"pred_boxes": pred}, targets, indices, float(d["num_boxes"]))
        grad, = torch.autograd.grad(out["loss_bbox"] + out["loss_giou"], pred)
        assert_close(out["loss_bbox"], d["loss_bbox"], 1e-4, "loss_bbox")
        assert_close(out["loss_giou"], d["loss_giou"], 1e-4, "loss_giou")
        assert_close(grad[0], d["grad_src"], 1e-4, "grad_src")


def test_compile_fullgraph_with_changing_sizes_gives_eagers_bits():
    import devis_amd

    def cost(x, b, l, t):
        return devis_amd.match_cost(x, b, l, t, l1="sum", **WEIGHTS)

    compiled_cost = torch.compile(cost, fullgraph=True)
    compiled_terms = torch.compile(devis_amd.box_loss_terms, fullgraph=True)
    for shape in ((1, 3, 7, 4, 5), (1, 3, 11, 6, 5), (1, 3, 50, 9, 5)):                  # R and T change: dynamic by themselves
        ops = on_gpu(cost_case(shape, torch.float32)[0]) if shape in SHAPES else None
        if ops is None:
            L, Fr, R, T, C = shape
            g = torch.Generator().manual_seed(R)
            ops = on_gpu(((3 * torch.randn(L, Fr, R, C, generator=g)), boxes_of(g, L, Fr, R).float(),
                          torch.randint(0, C, (T, Fr), generator=g), boxes_of(g, T, Fr).float()))
        got, want = compiled_cost(*ops), cost(*ops)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for N in (9, 5, 300):
        src, tgt = box_case(N, torch.float32)
        g1 = torch.randn(N, device=DEV)
        s, t = src.to(DEV).requires_grad_(True), tgt.to(DEV)
        want = devis_amd.box_loss_terms(s, t)
        want_grad, = torch.autograd.grad(list(want), s, [g1, 2 * g1])
        s = src.to(DEV).requires_grad_(True)
        got = compiled_terms(s, t)
        grad, = torch.autograd.grad(list(got), s, [g1, 2 * g1])
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(grad, want_grad)


def test_export_runs_the_operators():
    import devis_amd

    class Both(torch.nn.Module):
        def forward(self, x, b, l, t, src, tgt):
            cost, status = devis_amd.match_cost(x, b, l, t, **WEIGHTS)
            l1, giou = devis_amd.box_loss_terms(src, tgt)
            return cost, status, l1, giou

    ops = on_gpu(cost_case(SHAPES[0], torch.float32)[0])
    src, tgt = (t.to(DEV) for t in box_case(9, torch.float32))
    ep = torch.export.export(Both(), ops + (src, tgt))
    got, want = ep.module()(*ops, src, tgt), Both()(*ops, src, tgt)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_hip_graph_replay_with_changed_inputs_gives_the_changed_result():
    import devis_amd
    from devis_amd import ops as O
    ops = [t.clone() for t in on_gpu(cost_case(SHAPES[0], torch.float32)[0])]
    src, tgt = (t.to(DEV).clone() for t in box_case(9, torch.float32))
    g1 = torch.ones(9, device=DEV)

    def call():
        cost, status = devis_amd.match_cost(*ops, **WEIGHTS)
        l1, giou = devis_amd.box_loss_terms(src, tgt)
        return cost, status, l1, giou, O.box_loss_terms_backward(g1, g1, src, tgt)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()          # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    new = on_gpu(cost_case(SHAPES[0], torch.float32)[0])
    ops[0].copy_(new[0].flip(2))
    ops[3].copy_(new[3].flip(0))
    ops[3][1, 1, 2] = -0.25                     # and a degenerate target box: the status is zeroed and counted per replay
    src2, tgt2 = box_case(9, torch.float32, seed=5)
    src.copy_(src2)
    tgt.copy_(tgt2)
    graph.replay()
    torch.cuda.synchronize()
    assert out[1].tolist() == [0, 1, 0]
    graph.replay()
    torch.cuda.synchronize()
    assert out[1].tolist() == [0, 1, 0]
    assert all(torch.equal(a, b) for a, b in zip(out, call()))
    want = boxmatch_oracle.box_loss_terms(src2.double(), tgt2.double(), grads=(torch.ones(9, dtype=F64),) * 2)
    for got, w, what in zip(out[2:], want, ("l1", "giou", "grad_src")):
        assert_close(got, w, 1e-4, "graph replay " + what)
