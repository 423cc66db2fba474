"""GPU tests of the linear sum assignment solver (include/assign.h): the indices against scipy on the same cost in double --
with ``==``: the method and its arithmetic are scipy's, so on a cost whose optimum is unique there is nothing to tolerate --
and against the numpy oracle of tests/assign_oracle.py, which shares the kernel's tie rule, where it is not unique.  The shapes are those
of tests/test_assign_cpu.py, where WIDE_VARIANTS states which instantiation of the kernel (columns per lane, staged or not,
transposed or not) each of the wide ones selects."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import assign_oracle
from test_assign_cpu import (LIMIT, RANK_ONE, SHAPES, TIED, WIDE, WIDE_RANK_ONE, WIDE_TIED, generic_case, rank_one_case,
                             special_cases, tied_case)
from test_boxmatch_cpu import devis_call, load_fixture, modules, same_tensors
from test_boxmatch_gpu import cost_case, gpu_targets, on_gpu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64]
ids_of_shape = lambda s: "x".join(map(str, s))      # noqa: E731
ids_of_dtype = lambda d: str(d).split(".")[1]       # noqa: E731

_F64_CASES = {}


def float64_case(shape, k):
    """A float64 standard-normal cost (entries no float32 holds) and scipy's answer: computed once, read only."""
    if (shape, k) not in _F64_CASES:
        c = np.random.RandomState(77 * shape[0] + shape[1] + 7919 * k).standard_normal(shape)
        _F64_CASES[shape, k] = (c, linear_sum_assignment(c))
    return _F64_CASES[shape, k]


def solve(cost):
    """devis_amd.linear_assignment of a numpy [L, R, T] or [R, T] cost -> numpy (rows, cols, status)."""
    import devis_amd
    c = torch.from_numpy(np.ascontiguousarray(cost))
    rows, cols, status = devis_amd.linear_assignment((c if c.dim() == 3 else c[None]).to(DEV))
    assert rows.dtype == cols.dtype == torch.int64 and status.dtype == torch.int32 and rows.device == cols.device == status.device
    assert rows.is_cuda and tuple(status.shape) == (2,)
    return rows.cpu().numpy(), cols.cpu().numpy(), status.cpu().numpy()


def assert_pairs(got_rows, got_cols, want, what):
    assert got_rows.tolist() == want[0].tolist() and got_cols.tolist() == want[1].tolist(), what


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_of_dtype)
@pytest.mark.parametrize("shape", SHAPES + WIDE, ids=ids_of_shape)
def test_indices_equal_scipys_for_one_problem_and_for_three(shape, dtype):
    cases = [generic_case(shape, k) if dtype == torch.float32 else float64_case(shape, k) for k in range(3)]
    rows, cols, status = solve(cases[0][0])
    assert rows.shape == cols.shape == (1, min(shape)) and status.tolist() == [0, 0]
    assert_pairs(rows[0], cols[0], cases[0][1], "L = 1")
    rows, cols, status = solve(np.stack([c for c, _ in cases]))
    assert rows.shape == (3, min(shape)) and status.tolist() == [0, 0]
    for l, (_, want) in enumerate(cases):
        assert_pairs(rows[l], cols[l], want, "problem %d of 3" % l)


def test_the_largest_problem_equals_scipys():
    """1024 x 1024 in float32, one problem: 16 columns per lane, none of them dead, and both index fields of the candidate
    key up to 1023."""
    c, want = generic_case(LIMIT)
    rows, cols, status = solve(c)
    assert rows.shape == cols.shape == (1, 1024) and status.tolist() == [0, 0]
    assert_pairs(rows[0], cols[0], want, LIMIT)
    assert int(cols.max()) == 1023 and sorted(cols[0].tolist()) == list(range(1024))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_of_dtype)
@pytest.mark.parametrize("shape", RANK_ONE + [(300, 25)] + WIDE_RANK_ONE, ids=ids_of_shape)
def test_the_rank_one_family_is_solved_exactly(shape, dtype):
    """Every augmentation walks the whole matching made so far: n(n+1)/2 steps, the bound of the kernel's counted loops.
    25 x 300 and 300 x 25 hold several columns per lane in both orientations; 130 x 130 and 129 x 200 walk back along a path
    that crosses the column slots of a lane, with the rows in three rounds of 64 lanes."""
    if shape == (300, 25):
        c = np.ascontiguousarray(rank_one_case((25, 300))[0].T)
        want = linear_sum_assignment(c.astype(np.float64))
    else:
        c, want = rank_one_case(shape)
    rows, cols, status = solve(c.astype(np.float32 if dtype == torch.float32 else np.float64))
    assert status.tolist() == [0, 0]
    assert_pairs(rows[0], cols[0], want, shape)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_of_dtype)
@pytest.mark.parametrize("shape", TIED + WIDE_TIED, ids=ids_of_shape)
def test_tied_costs_equal_the_oracle_and_scipys_total(shape, dtype):
    c, want, total = tied_case(shape)
    rows, cols, status = solve(c.astype(np.float32 if dtype == torch.float32 else np.float64))
    assert status.tolist() == [0, 0]
    assert_pairs(rows[0], cols[0], want, shape)
    assert float(c[rows[0], cols[0]].sum()) == total


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_of_dtype)
def test_infinite_and_invalid_entries_in_one_call(dtype):
    cost, verdicts = special_cases()
    cost = cost.astype(np.float32 if dtype == torch.float32 else np.float64)
    if dtype == torch.float32:
        verdicts = [assign_oracle.solve(c) for c in cost]
    rows, cols, status = solve(cost)
    assert status.tolist() == [2, 1]                        # a NaN and a -inf; a column of +inf
    for l in (0, 1):                                        # clean; +inf entries that leave it feasible: as scipy solves them
        want = linear_sum_assignment(cost[l].astype(np.float64))
        assert_pairs(rows[l], cols[l], want, l)
        assert_pairs(rows[l], cols[l], verdicts[l], l)
    for l in (2, 3, 4):
        assert isinstance(verdicts[l], str) and rows[l].tolist() == cols[l].tolist() == [0, 1, 2, 3], l
    alone = solve(cost[0])
    assert alone[2].tolist() == [0, 0] and np.array_equal(alone[0][0], rows[0]) and np.array_equal(alone[1][0], cols[0])
    # the transposed orientation too: a row of +inf leaves 4 x 5 infeasible, one +inf entry does not
    t = np.ascontiguousarray(cost[:3].transpose(0, 2, 1))
    rows, cols, status = solve(t)
    assert status.tolist() == [0, 1] and rows[2].tolist() == cols[2].tolist() == [0, 1, 2, 3]
    for l in (0, 1):
        assert_pairs(rows[l], cols[l], linear_sum_assignment(t[l].astype(np.float64)), ("transposed", l))


def test_two_runs_are_bitwise_equal_and_a_problem_is_the_same_alone_and_among_others():
    cases = [rank_one_case((24, 24))[0], tied_case((9, 9))[0]]
    for shape in ((50, 4), (9, 65), (65, 9)):
        batch = np.stack([generic_case(shape, k)[0] for k in range(3)])
        first, second = solve(batch), solve(batch)
        assert all(np.array_equal(a, b) for a, b in zip(first, second))
        for l in range(3):
            alone = solve(batch[l])
            assert np.array_equal(alone[0][0], first[0][l]) and np.array_equal(alone[1][0], first[1][l])
    for c in cases:
        many = solve(np.stack([c, c[::-1].copy(), c]))
        alone = solve(c)
        assert all(np.array_equal(a, b) for a, b in zip(solve(c), alone))
        assert np.array_equal(many[0][0], alone[0][0]) and np.array_equal(many[1][0], alone[1][0])
        assert np.array_equal(many[0][2], alone[0][0]) and np.array_equal(many[1][2], alone[1][0])


def test_empty_problems_launch_nothing(monkeypatch):
    import devis_amd
    from devis_amd import _assign
    monkeypatch.setattr(_assign, "solve", lambda *a: (_ for _ in ()).throw(AssertionError("a kernel call was made")))
    for shape in ((0, 7, 4), (3, 0, 4), (3, 7, 0)):
        rows, cols, status = devis_amd.linear_assignment(torch.zeros(shape, device=DEV))
        assert tuple(rows.shape) == tuple(cols.shape) == (shape[0], min(shape[1:])) and status.tolist() == [0, 0]


def test_one_graph_capture_of_cost_and_assignment_replays_to_the_eager_result():
    import devis_amd
    weights = dict(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)
    shape = (3, 6, 50, 9, 40)                   # (L, F, R, T, C)
    ops = [t.clone() for t in on_gpu(cost_case(shape, torch.float32)[0])]

    def call():
        cost, cost_status = devis_amd.match_cost(*ops, **weights)
        return (cost, cost_status) + devis_amd.linear_assignment(cost)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()          # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    new = on_gpu(cost_case(shape, torch.float32)[0])
    ops[0].copy_(new[0].flip(2))
    ops[3].copy_(new[3].flip(0))
    graph.replay()
    torch.cuda.synchronize()
    eager = call()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    assert out[1].tolist() == [0, 0, 0] and out[4].tolist() == [0, 0]
    cost = out[0].double().cpu().numpy()
    for l in range(3):
        assert_pairs(out[2][l].cpu().numpy(), out[3][l].cpu().numpy(), linear_sum_assignment(cost[l]), l)
    ops[0][1, 2, 3, :] = float("nan")           # and a row of NaN logits: the status is zeroed and counted per replay
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert out[4].tolist() == [1, 0] and out[2][1].tolist() == out[3][1].tolist() == list(range(9))
        assert torch.equal(out[2][0], eager[2][0]) and torch.equal(out[3][2], eager[3][2])


@pytest.mark.parametrize("batch_aux", [False, True], ids=["per call", "batch_aux"])
def test_patched_devis_matcher_does_not_synchronise_and_returns_the_host_paths_values(batch_aux):
    import devis_amd
    for name in ("boxmatch_devis_mean", "boxmatch_devis_sum"):
        d = load_fixture(name)
        top, targets = devis_call(d)
        g = torch.Generator().manual_seed(3)
        layer = lambda: {"pred_logits": (top["pred_logits"] + 0.5 * torch.randn(top["pred_logits"].shape, generator=g, dtype=torch.float64)).float().to(DEV),      # noqa: E731,B023
                         "pred_boxes": (top["pred_boxes"] * (1 + 0.1 * torch.rand(top["pred_boxes"].shape, generator=g, dtype=torch.float64))).float().to(DEV)}      # noqa: B023
        outputs = {k: v.float().to(DEV) for k, v in top.items()}
        if batch_aux:
            outputs["aux_outputs"] = [layer() for _ in range(5)]
        targets = gpu_targets(targets)
        results = {}
        for mode in (False, True):
            crit, match = modules()
            matcher = match.DeVISHungarianMatcher(d)
            run = (lambda: crit.SetCriterion(matcher).forward(outputs, targets)) if batch_aux else (lambda: [matcher(outputs, targets)])      # noqa: B023
            previous = devis_amd.patch_criterion(crit, match, batch_aux=batch_aux, gpu_assignment=mode)
            try:
                results[mode] = run()                       # (loads the library, warms the allocator)
                if mode:
                    torch.cuda.synchronize()
                    torch.cuda.set_sync_debug_mode("error")
                    try:
                        results[mode] = run()               # a synchronising call would raise here
                    finally:
                        torch.cuda.set_sync_debug_mode("default")
                    assert matcher.last_match_status.is_cuda and matcher.last_match_status.tolist() == [0] * 5
                    devis_amd.raise_on_match_status(matcher.last_match_status)
            finally:
                devis_amd.unpatch_criterion(crit, match, previous)
        assert len(results[True]) == len(results[False]) == (6 if batch_aux else 1)
        for got, want in zip(results[True], results[False]):
            (index_i, index_j, index_valid), = got
            assert index_i.is_cuda and index_j.is_cuda and index_valid.device == targets[0]["valid"].device
            assert want[0][0].device.type == "cpu"
            assert same_tensors((index_i.cpu(), index_j.cpu(), index_valid), want[0])
        first = results[True][0][0]
        assert same_tensors(tuple(t.cpu() for t in first), (d["index_i"], d["index_j"], d["index_valid"]))


def test_raise_on_match_status_raises_the_four_kinds():
    import devis_amd
    d = load_fixture("boxmatch_devis_mean")
    crit, match = modules()
    outputs, targets = devis_call(d)
    outputs, targets = {k: v.float().to(DEV) for k, v in outputs.items()}, gpu_targets(targets)
    matcher = match.DeVISHungarianMatcher(d)
    previous = devis_amd.patch_criterion(crit, match, gpu_assignment=True)
    try:
        bad = dict(targets[0], labels=targets[0]["labels"].clone())
        bad["labels"][4] = 5
        matcher(outputs, [bad])             # (the label's target has NaN costs: the assignment counts its problem as well)
        assert matcher.last_match_status.tolist() == [0, 0, 1, 1, 0]
        with pytest.raises(IndexError, match="1 target label\\(s\\) outside \\[0, 5\\)"):
            devis_amd.raise_on_match_status(matcher.last_match_status, num_classes=5)
        bad = dict(targets[0], boxes=targets[0]["boxes"].clone())
        bad["boxes"][3, 2] = -0.1
        ((index_i, index_j, _),) = matcher(outputs, [bad])
        assert matcher.last_match_status.tolist() == [0, 1, 0, 0, 0] and int(index_i.max()) < 21 and int(index_j.max()) < 12
        with pytest.raises(AssertionError, match="0 prediction and 1 target box"):
            devis_amd.raise_on_match_status(matcher.last_match_status)
    finally:
        devis_amd.unpatch_criterion(crit, match, previous)
    cost = torch.from_numpy(special_cases()[0]).to(DEV)
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        devis_amd.raise_on_match_status(devis_amd.linear_assignment(cost)[2])
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        devis_amd.raise_on_match_status(torch.cat([torch.zeros(3, dtype=torch.int32, device=DEV), devis_amd.linear_assignment(cost[:3])[2]]))
    devis_amd.raise_on_match_status(devis_amd.linear_assignment(cost[:2])[2])
