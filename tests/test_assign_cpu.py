"""CPU tests of the linear sum assignment solver: the numpy oracle of tests/assign_oracle.py against scipy, the C ABI of
include/assign.h (exports, version, argument errors -- no compute calls), the host code (shape checks, CPU tensors raise), the
fake-tensor paths, and patch_criterion(gpu_assignment=True) on stand-in matcher and criterion classes with both operators
replaced by their oracles.  The kernel itself is tests/test_assign_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import assign_oracle
import boxmatch_oracle
from conftest import ROOT
from test_boxmatch_cpu import devis_call, image_call, load_fixture, modules, same_tensors

F64 = torch.float64
# the generic shapes (R, T): both orientations, one and several columns per lane, a side that is no multiple of 64, the limit
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (7, 7), (50, 4), (4, 50), (64, 9), (65, 9), (9, 65), (128, 3), (1024, 2), (2, 1024)]
RANK_ONE = [(7, 7), (24, 24), (25, 300), (65, 65)]
TIED = [(12, 5), (5, 12), (9, 9)]
# The wide shapes: a longer side above 128 (4, 8 and 16 columns per lane), a shorter side above 65 (several rounds of 64 lanes
# over the rows, a path back across several column slots), cost blocks too large to stage, rows above 63 in the candidate key.
# WIDE_VARIANTS states the instantiation each of them selects.
WIDE = [(150, 150), (130, 90), (90, 130), (200, 260), (40, 300), (300, 40), (513, 70), (70, 513)]
LIMIT = (1024, 1024)                    # one float32 problem: both key fields at full width
WIDE_RANK_ONE = [(130, 130), (129, 200)]
WIDE_TIED = [(70, 130), (130, 70), (140, 140)]

# csrc/assign.hip restated: launch_k's steps of the longer side, kStageBytes, and `transposed = R > T`
LANE_COLUMNS = ((64, 1), (128, 2), (256, 4), (512, 8), (1024, 16))
STAGE_BYTES = 48 << 10


def variant(shape, itemsize):
    """(K, staged, transposed) of solve_kernel for a cost of ``shape`` with entries of ``itemsize`` bytes."""
    n, m = min(shape), max(shape)
    return next(k for limit, k in LANE_COLUMNS if m <= limit), n * m * itemsize <= STAGE_BYTES, shape[0] > shape[1]


# shape -> (the float32 variant, the float64 variant)
WIDE_VARIANTS = {
    (150, 150): ((4, False, False), (4, False, False)),
    (130, 90): ((4, True, True), (4, False, True)),
    (90, 130): ((4, True, False), (4, False, False)),
    (200, 260): ((8, False, False), (8, False, False)),
    (40, 300): ((8, True, False), (8, False, False)),
    (300, 40): ((8, True, True), (8, False, True)),
    (513, 70): ((16, False, True), (16, False, True)),
    (70, 513): ((16, False, False), (16, False, False)),
}

_CASES = {}


def generic_case(shape, k=0):
    """A float32 standard-normal cost of ``shape`` from a fixed seed and scipy's answer on it: computed once, read only."""
    key = ("generic", shape, k)
    if key not in _CASES:
        rng = np.random.RandomState(1000 * shape[0] + shape[1] + 7919 * k)
        c = rng.standard_normal(shape).astype(np.float32)
        _CASES[key] = (c, linear_sum_assignment(c.astype(np.float64)))
    return _CASES[key]


def rank_one_case(shape):
    key = ("rank one", shape)
    if key not in _CASES:
        c = assign_oracle.rank_one(*shape, seed=shape[0] + shape[1])
        _CASES[key] = (c, linear_sum_assignment(c.astype(np.float64)))
    return _CASES[key]


def tied_case(shape):
    """Integer costs in {0, 1, 2}: the optimum is far from unique.  (cost, the oracle's answer, scipy's total)."""
    key = ("tied", shape)
    if key not in _CASES:
        c = np.random.RandomState(shape[0] * 31 + shape[1]).randint(0, 3, size=shape).astype(np.float32)
        rows, cols = linear_sum_assignment(c.astype(np.float64))
        _CASES[key] = (c, assign_oracle.solve(c), float(c[rows, cols].sum()))
    return _CASES[key]


def special_cases():
    """Five 5 x 4 problems for one call: clean, a +inf entry that leaves it feasible, a column of +inf (no assignment of the 4
    columns exists), a NaN, a -inf.  Returns (cost float64 [5, 5, 4], what the oracle says of each)."""
    base = np.random.RandomState(5).standard_normal((5, 5, 4))
    base[1, 2, 1] = np.inf
    base[1, 0, 0] = np.inf
    base[2, :, 1] = np.inf
    base[3, 4, 3] = np.nan
    base[4, 0, 2] = -np.inf
    return base, [assign_oracle.solve(c) for c in base]


# ---- oracle ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES + WIDE, ids=lambda s: "x".join(map(str, s)))
def test_oracle_gives_scipys_indices_on_generic_costs(shape):
    for k in range(3):
        c, (rows, cols) = generic_case(shape, k)
        got = assign_oracle.solve(c)
        assert got[0].dtype == got[1].dtype == np.int64
        assert np.array_equal(got[0], rows) and np.array_equal(got[1], cols), (shape, k)


@pytest.mark.parametrize("shape", RANK_ONE + WIDE_RANK_ONE, ids=lambda s: "x".join(map(str, s)))
def test_oracle_gives_scipys_indices_on_the_rank_one_family(shape):
    c, (rows, cols) = rank_one_case(shape)
    got = assign_oracle.solve(c)
    assert np.array_equal(got[0], rows) and np.array_equal(got[1], cols)
    n, m = min(shape), max(shape)
    # sorted factors: the optimum pairs the n largest of the long side with the short side in order
    mine, in_order = got[1] if shape[0] <= shape[1] else got[0], np.arange(m - n, m)
    if shape in RANK_ONE:
        assert np.array_equal(mine, in_order)
    else:
        # The entries are products rounded to float32.  At these sizes two neighbouring factors can lie closer than that
        # rounding (129 x 200 has one such pair): the optimum of the rounded cost -- scipy's and the oracle's alike -- may then
        # exchange neighbours, and is no dearer than the pairing in order.
        wide = c.astype(np.float64) if shape[0] <= shape[1] else c.astype(np.float64).T
        assert np.abs(mine - in_order).max() <= 1 and sorted(mine.tolist()) == in_order.tolist()
        assert wide[np.arange(n), mine].sum() <= wide[np.arange(n), in_order].sum()


@pytest.mark.parametrize("shape", TIED + WIDE_TIED, ids=lambda s: "x".join(map(str, s)))
def test_oracle_total_equals_scipys_on_tied_costs(shape):
    c, (rows, cols), total = tied_case(shape)
    n = min(shape)
    assert len(rows) == n and np.all(np.diff(rows) > 0) and len(set(cols.tolist())) == n
    assert float(c[rows, cols].sum()) == total


def test_the_wide_shapes_select_every_variant_of_the_kernel_with_four_or_more_columns_per_lane():
    """Which (K, staged, transposed) each wide shape runs, from the thresholds of csrc/assign.hip restated above: when one of
    them moves, this says which variant lost its cases.  The solver's GPU tests run every shape named here in both types,
    except LIMIT (float32 only)."""
    source = open(os.path.join(ROOT, "devis_amd", "csrc", "assign.hip")).read()
    assert "constexpr int kStageBytes = 48 << 10;" in source and "const bool transposed = R > Tn;" in source
    assert re.findall(r"if \(m <= (\d+)\) return launch<T, (\d+)>", source) == [(str(m), str(k)) for m, k in LANE_COLUMNS[:-1]]
    assert "return launch<T, 16>" in source and LANE_COLUMNS[-1] == (1024, 16)
    assert set(WIDE_VARIANTS) == set(WIDE)
    for shape in WIDE:
        assert (variant(shape, 4), variant(shape, 8)) == WIDE_VARIANTS[shape], shape
    assert variant(LIMIT, 4) == (16, False, False)
    reached = {v for pair in WIDE_VARIANTS.values() for v in pair}
    # a staged block with 16 columns per lane has a shorter side of at most 23: (1024, 2) and (2, 1024) of SHAPES are those
    assert variant((1024, 2), 4) == variant((1024, 2), 8) == (16, True, True) and (1024, 2) in SHAPES
    assert variant((2, 1024), 4) == variant((2, 1024), 8) == (16, True, False) and (2, 1024) in SHAPES
    for k in (4, 8, 16):
        for staged in (True, False):
            for transposed in (True, False):
                assert (k, staged, transposed) in reached or (k, staged) == (16, True), (k, staged, transposed)
    # what the other families add: a shorter side above 64 under 2, 4 and more columns per lane, ties across the slots
    assert [variant(s, 4)[0] for s in WIDE_RANK_ONE] == [4, 4] and [variant(s, 4)[0] for s in WIDE_TIED] == [4, 4, 4]
    assert all(min(s) > 65 for s in WIDE_RANK_ONE + WIDE_TIED) and {variant(s, 4)[2] for s in WIDE_TIED} == {True, False}


def test_oracle_classifies_invalid_and_infeasible_inputs_as_scipy_does():
    cost, verdicts = special_cases()
    for c, verdict, message in zip(cost, verdicts, (None, None, "cost matrix is infeasible", "invalid numeric entries",
                                                    "invalid numeric entries")):
        if message is None:
            rows, cols = linear_sum_assignment(c)
            assert np.array_equal(verdict[0], rows) and np.array_equal(verdict[1], cols)
        else:
            with pytest.raises(ValueError, match=message):
                linear_sum_assignment(c)
            assert verdict == (assign_oracle.INFEASIBLE if "infeasible" in message else assign_oracle.INVALID)
    rows, cols, status = assign_oracle.solve_batch(cost)
    assert status.tolist() == [2, 1] and status.dtype == np.int32
    for l in (2, 3, 4):
        assert rows[l].tolist() == cols[l].tolist() == [0, 1, 2, 3]
    assert np.array_equal(cols[0], verdicts[0][1]) and np.array_equal(cols[1], verdicts[1][1])
    empty = assign_oracle.solve(np.zeros((0, 4)))
    assert empty[0].shape == empty[1].shape == (0,)


# ---- library ---------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_assign_h_declares_and_versions_agree():
    from devis_amd import _assign, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "assign.h")).read()
    declared = set(re.findall(r"\b(assign_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_assign.EXPORTED_SYMBOLS) and len(declared) == 3
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _assign.load()
    assert lib.assign_version() == _assign.ASSIGN_ABI_VERSION == int(re.search(r"#define ASSIGN_ABI_VERSION (\d+)", header).group(1))
    assert int(re.search(r"#define ASSIGN_MAX_SIDE (\d+)", header).group(1)) == _assign.MAX_SIDE == 1024
    assert dict(re.findall(r"ASSIGN_(F32|F64) = (\d)", header)) == {"F32": str(_assign.F32), "F64": str(_assign.F64)}
    for stated in ("left to right", "has no row", "lowest column index", "counted", "(k, k)"):      # the contract is stated
        assert stated in header, stated
    assert os.path.join(build.include_dir(), "assign.h") in build._headers()
    assert any(s.endswith("assign.hip") for s in build.sources())
    assert "assign.h" in open(os.path.join(ROOT, "setup.py")).read() and "assign.h" in build.include_dir.__doc__


def test_assign_argument_errors_without_gpu():
    from devis_amd import _assign
    lib = _assign.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.assign_last_error

    def solve(dtype=0, cost=p, L=1, R=7, T=4, rows=p, cols=p, status=p):
        return lib.assign_solve(dtype, cost, L, R, T, rows, cols, status, None)

    for bad in (2, 3, 9, -1):            # (the 16-bit codes of the other operators included)
        assert solve(dtype=bad) == -1 and b"dtype" in err()
    for bad in (dict(R=1025), dict(T=1025), dict(R=1025, T=0)):
        assert solve(**bad) == -1 and b"exceeds the limit of 1024" in err(), bad
    for bad in (dict(L=-1), dict(R=-1), dict(T=-1)):
        assert solve(**bad) == -1 and b"negative" in err(), bad
    assert solve(L=4096, R=1024, T=1024) == -1 and b"31 bits" in err()
    for name in ("cost", "rows", "cols", "status"):
        assert solve(**{name: None}) == -1 and b"null pointer" in err(), name
    # nothing to solve: nothing is launched, nothing is dereferenced
    for empty in (dict(L=0), dict(R=0), dict(T=0)):
        assert solve(cost=None, rows=None, cols=None, status=None, **empty) == 0 and err() == b""


# ---- host ------------------------------------------------------------------------------------------------------------

def test_operator_raises_on_cpu_tensors_and_on_bad_arguments_before_any_launch(monkeypatch):
    import devis_amd
    from devis_amd import _assign
    from devis_amd.functions import assignment as G

    def no_launch(*a, **k):
        raise AssertionError("a kernel call was made")

    monkeypatch.setattr(_assign, "solve", no_launch)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.linear_assignment(torch.zeros(2, 7, 4))
    with pytest.raises(RuntimeError, match="cost requires a gradient"):
        devis_amd.linear_assignment(torch.zeros(2, 7, 4, requires_grad=True))
    for name in ("linear_assignment", "raise_on_match_status"):
        assert name in devis_amd.__all__
    assert devis_amd.linear_assignment is devis_amd.ops.linear_assignment
    assert devis_amd.raise_on_match_status is devis_amd.argument_builders.raise_on_match_status
    meta = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="meta")      # noqa: E731
    assert G.check_cost(meta(2, 7, 4)) == (2, 7, 4) and G.check_cost(meta(0, 1024, 1024, dtype=F64)) == (0, 1024, 1024)
    assert G.fits(1024, 1) and not G.fits(1025, 1) and not G.fits(3, 1025)
    bad = [("cost must be \\[L, R, T\\]", lambda: G.check_cost(meta(7, 4))),
           ("float32 or float64", lambda: G.check_cost(meta(2, 7, 4, dtype=torch.bfloat16))),
           ("float32 or float64", lambda: G.check_cost(meta(2, 7, 4, dtype=torch.int64))),
           ("exceeds the limit of 1024", lambda: G.check_cost(meta(1, 1025, 4))),
           ("exceeds the limit of 1024", lambda: G.check_cost(meta(1, 4, 2000)))]
    for match, call in bad:
        with pytest.raises(RuntimeError, match=match):
            call()


def test_raise_on_match_status_raises_the_four_kinds_from_host_counts():
    import devis_amd
    check = devis_amd.raise_on_match_status
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    check(None)
    check(i32(0, 0, 0, 0, 0))
    check(i32(0, 0, 0))
    check(i32(0, 0))
    with pytest.raises(IndexError, match="2 target label\\(s\\) outside \\[0, 5\\)"):
        check(i32(1, 1, 2, 1, 1), num_classes=5)                # the order of the host path: labels first
    with pytest.raises(IndexError, match="outside the classes"):
        check(i32(0, 0, 1))
    with pytest.raises(AssertionError, match="1 prediction and 0 target box"):
        check(i32(1, 0, 0, 1, 1))
    with pytest.raises(AssertionError, match="0 prediction and 3 target box"):
        check(i32(0, 3, 0, 0, 0))
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        check(i32(0, 0, 0, 2, 1))
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        check(i32(0, 0, 0, 0, 1))
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        check(i32(0, 1))
    with pytest.raises(ValueError, match="5, 3 or 2 counts"):
        check(i32(0, 0, 0, 0))


# ---- fake-tensor paths -----------------------------------------------------------------------------------------------

def _nodes(graph, name):
    return [n for n in graph.nodes if n.op == "call_function" and name in str(n.target)]


def test_make_fx_with_fake_tensors_gives_one_op_node():
    from torch.fx.experimental.proxy_tensor import make_fx
    from devis_amd import ops
    for dtype in (torch.float32, F64):
        for shape, n in (((6, 50, 4), 4), ((1, 3, 9), 3)):
            gm = make_fx(ops.linear_assignment_op, tracing_mode="fake")(torch.empty(*shape, dtype=dtype, device="meta"))
            node, = _nodes(gm.graph, "linear_assignment")
            rows, cols, status = node.meta["val"]
            assert tuple(rows.shape) == tuple(cols.shape) == (shape[0], n) and rows.dtype == cols.dtype == torch.int64
            assert tuple(status.shape) == (2,) and status.dtype == torch.int32
    with pytest.raises(Exception, match="float32 or float64"):
        make_fx(ops.linear_assignment_op, tracing_mode="fake")(torch.empty(2, 7, 4, dtype=torch.float16, device="meta"))


@pytest.mark.parametrize("dynamic", [False, True])
def test_export_gives_one_op_node_for_static_and_dynamic_L(dynamic):
    import devis_amd

    class Solve(torch.nn.Module):
        def forward(self, cost):
            return devis_amd.linear_assignment(cost)

    shapes = ({0: torch.export.Dim("L", min=2, max=64)},) if dynamic else None
    graph = torch.export.export(Solve(), (torch.empty(6, 50, 4, device="meta"),), dynamic_shapes=shapes).graph
    node, = _nodes(graph, "linear_assignment")
    rows = node.meta["val"][0]
    assert len(rows.shape) == 2 and rows.shape[1] == 4
    assert not isinstance(rows.shape[0], int) if dynamic else rows.shape[0] == 6


# ---- patch_criterion(gpu_assignment=True) ----------------------------------------------------------------------------

def oracle_assignment(cost):
    rows, cols, status = assign_oracle.solve_batch(cost.numpy())
    return torch.from_numpy(rows), torch.from_numpy(cols), torch.from_numpy(status)


@pytest.fixture()
def stubbed(monkeypatch):
    """(criterion module, matcher module, calls): both operators replaced by their oracles, which note their calls; the host
    solver replaced by one that notes its calls too."""
    from devis_amd import argument_builders, ops
    calls = []
    monkeypatch.setattr(ops, "match_cost", lambda *a, **k: calls.append(("cost", tuple(a[0].shape))) or boxmatch_oracle.match_cost(*a, **k))
    monkeypatch.setattr(ops, "linear_assignment", lambda c: calls.append(("assign", tuple(c.shape))) or oracle_assignment(c))
    solver = argument_builders._solver()
    monkeypatch.setattr(argument_builders, "_solver", lambda: lambda c: calls.append(("scipy", tuple(c.shape))) or solver(c))
    crit, match = modules()
    return crit, match, calls


def test_patch_criterion_with_gpu_assignment_sets_and_restores_the_methods():
    import devis_amd
    crit, match = modules()
    theirs = (crit.SetCriterion.loss_boxes, crit.SetCriterion.forward, match.DeVISHungarianMatcher.forward, match.HungarianMatcher.forward)
    current = lambda: (crit.SetCriterion.loss_boxes, crit.SetCriterion.forward, match.DeVISHungarianMatcher.forward,      # noqa: E731
                       match.HungarianMatcher.forward)
    previous = devis_amd.patch_criterion(crit, match, gpu_assignment=True)
    assert previous == {"loss_boxes": theirs[0], "devis_forward": theirs[2], "image_forward": theirs[3]}
    assert match.DeVISHungarianMatcher.forward.indices_of is devis_amd.argument_builders._devis_indices_on_device
    assert match.HungarianMatcher.forward.indices_of is devis_amd.argument_builders._image_indices
    assert crit.SetCriterion.forward is theirs[1]
    devis_amd.unpatch_criterion(crit, match, previous)
    assert current() == theirs
    previous = devis_amd.patch_criterion(crit, match, batch_aux=True, gpu_assignment=True)
    assert previous["criterion_forward"] is theirs[1] and crit.SetCriterion.forward is not theirs[1]
    devis_amd.unpatch_criterion(crit, match, previous)
    assert current() == theirs
    previous = devis_amd.patch_criterion(crit, match)             # the default stays the host path
    assert match.DeVISHungarianMatcher.forward.indices_of is devis_amd.argument_builders._devis_indices
    devis_amd.unpatch_criterion(crit, match, previous)
    assert current() == theirs


@pytest.mark.parametrize("name", ["boxmatch_devis_mean", "boxmatch_devis_sum"])
def test_stubbed_devis_matcher_returns_the_reference_values_without_the_host_solver(name, stubbed):
    import devis_amd
    crit, match, calls = stubbed
    d = load_fixture(name)
    previous = devis_amd.patch_criterion(crit, match, gpu_assignment=True)
    try:
        matcher = match.DeVISHungarianMatcher(d)
        out = matcher(*devis_call(d))
        assert isinstance(out, list) and len(out) == 1 and isinstance(out[0], tuple)
        assert same_tensors(out[0], (d["index_i"], d["index_j"], d["index_valid"]))
        assert calls == [("cost", (1, 3, 7, 5)), ("assign", (1, 7, 4))]
        assert matcher.last_match_status.dtype == torch.int32 and matcher.last_match_status.tolist() == [0] * 5
        devis_amd.raise_on_match_status(matcher.last_match_status)
        # nothing is raised by the matcher; the status tells
        outputs, targets = devis_call(d)
        bad = dict(targets[0], labels=targets[0]["labels"].clone())
        bad["labels"][4] = 5
        matcher(outputs, [bad])
        with pytest.raises(IndexError, match="1 target label\\(s\\) outside \\[0, 5\\)"):
            devis_amd.raise_on_match_status(matcher.last_match_status, num_classes=5)
        # the paths the shapes decide: no targets (no launch), the non-focal matcher (theirs)
        del calls[:]
        none = [{k: v[:2] for k, v in targets[0].items()}]                    # 2 // 3 == 0 targets
        (index_i, index_j, index_valid), = matcher(outputs, none)
        assert calls == [] and matcher.last_match_status is None
        assert same_tensors((index_i, index_j, index_valid), (torch.arange(3) * 7, torch.arange(3), torch.zeros(3, dtype=torch.bool)))
        assert match.DeVISHungarianMatcher(d, focal_loss=False)(*devis_call(d)) == "theirs" and calls == []
    finally:
        devis_amd.unpatch_criterion(crit, match, previous)


def test_a_shape_beyond_the_limits_takes_the_host_path(stubbed, monkeypatch):
    import devis_amd
    from devis_amd.functions import assignment as G
    crit, match, calls = stubbed
    monkeypatch.setattr(G, "MAX_SIDE", 6)                  # (the fixture has 7 queries)
    d = load_fixture("boxmatch_devis_mean")
    previous = devis_amd.patch_criterion(crit, match, gpu_assignment=True)
    try:
        matcher = match.DeVISHungarianMatcher(d)
        out = matcher(*devis_call(d))
        assert same_tensors(out[0], (d["index_i"], d["index_j"], d["index_valid"]))
        assert calls == [("cost", (1, 3, 7, 5)), ("scipy", (7, 4))] and matcher.last_match_status is None
    finally:
        devis_amd.unpatch_criterion(crit, match, previous)


def test_stubbed_batch_aux_makes_one_call_each_and_the_image_matcher_keeps_the_host_path(stubbed):
    import devis_amd
    crit, match, calls = stubbed
    d = load_fixture("boxmatch_devis_mean")
    top, targets = devis_call(d)
    g = torch.Generator().manual_seed(3)
    layer = lambda: {"pred_logits": top["pred_logits"] + 0.5 * torch.randn(top["pred_logits"].shape, generator=g, dtype=F64),      # noqa: E731
                     "pred_boxes": top["pred_boxes"] * (1 + 0.1 * torch.rand(top["pred_boxes"].shape, generator=g, dtype=F64))}
    outputs = dict(top, aux_outputs=[layer(), layer()])
    matcher = match.DeVISHungarianMatcher(d)
    previous = devis_amd.patch_criterion(crit, match, batch_aux=True)
    try:
        host = crit.SetCriterion(matcher).forward(outputs, targets)
    finally:
        devis_amd.unpatch_criterion(crit, match, previous)
    assert [c[0] for c in calls] == ["cost", "scipy", "scipy", "scipy"]
    del calls[:]
    previous = devis_amd.patch_criterion(crit, match, batch_aux=True, gpu_assignment=True)
    try:
        got = crit.SetCriterion(matcher).forward(outputs, targets)
        assert calls == [("cost", (3, 3, 7, 5)), ("assign", (3, 7, 4))]
        assert len(got) == len(host) == 3 and matcher.last_match_status.tolist() == [0] * 5
        for a, b in zip(got, host):
            assert len(a) == len(b) == 1 and same_tensors(a[0], b[0])
        assert same_tensors(got[0][0], (d["index_i"], d["index_j"], d["index_valid"]))
        # the image model's matcher: cost, transfer, scipy -- as without the keyword
        del calls[:]
        di = load_fixture("boxmatch_image")
        out = match.HungarianMatcher(di)(*image_call(di))
        assert calls == [("cost", (1, 1, 14, 5)), ("scipy", (7, 3)), ("scipy", (7, 2))]
        for b, pair in enumerate(out):
            assert same_tensors(pair, (di["index_i_%d" % b], di["index_j_%d" % b]))
    finally:
        devis_amd.unpatch_criterion(crit, match, previous)
