"""Numpy oracle of the linear sum assignment solver (include/assign.h): the shortest-augmenting-path method of Crouse 2016 that
``scipy.optimize.linear_sum_assignment`` documents, stated with the operator's tie rule -- among the unscanned columns of the
lowest shortest-path value one without a row wins, then the lowest index -- and the operator's arithmetic: double, the reduced
cost ``minv + c - u[i] - v[j]`` evaluated left to right.  Where the optimum is unique it gives scipy's indices; where it is
not it gives an optimum, and the kernel gives the same one bit for bit.  No torch, no GPU."""
import numpy as np

INVALID, INFEASIBLE = "invalid", "infeasible"        # scipy's "invalid numeric entries" / "infeasible"


def solve(cost):
    """``cost`` [R, T] -> ``(rows, cols)`` int64 [min(R, T)] ordered by ascending row, or INVALID (a NaN or a -inf entry) or
    INFEASIBLE (+inf entries leave no complete assignment)."""
    c = np.asarray(cost, dtype=np.float64)
    assert c.ndim == 2
    if min(c.shape) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    if np.isnan(c).any() or (c == -np.inf).any():
        return INVALID
    transposed = c.shape[0] > c.shape[1]
    if transposed:              # the shorter side is augmented, the longer one scanned
        c = c.T
    n, m = c.shape
    u, v = np.zeros(n), np.zeros(m)
    col4row, row4col = np.full(n, -1, np.int64), np.full(m, -1, np.int64)
    for cur in range(n):
        spc, path, scanned = np.full(m, np.inf), np.full(m, -1, np.int64), np.zeros(m, bool)
        minv, i, sink = 0.0, cur, -1
        for _ in range(cur + 1):            # a step scans one column; all but the last have one of the cur rows assigned so far
            r = ((minv + c[i]) - u[i]) - v
            better = ~scanned & (r < spc)
            spc[better], path[better] = r[better], i
            open_ = np.flatnonzero(~scanned)
            lowest = spc[open_].min()
            if not lowest < np.inf:
                return INFEASIBLE
            tied = open_[spc[open_] == lowest]
            free = tied[row4col[tied] == -1]
            j = int(free[0] if len(free) else tied[0])
            minv, scanned[j] = lowest, True
            if row4col[j] == -1:
                sink = j
                break
            i = int(row4col[j])
        assert sink >= 0
        for j in np.flatnonzero(scanned):           # the dual update (the sink's difference is 0)
            if row4col[j] != -1:
                u[row4col[j]] += minv - spc[j]
            v[j] -= minv - spc[j]
        u[cur] += minv
        j = sink
        for _ in range(cur + 1):                    # back along the path
            i = int(path[j])
            row4col[j] = i
            col4row[i], j = j, int(col4row[i])
            if i == cur:
                break
    if transposed:
        rows = np.flatnonzero(row4col != -1).astype(np.int64)
        return rows, row4col[rows].astype(np.int64)
    return np.arange(n, dtype=np.int64), col4row.astype(np.int64)


def solve_batch(cost):
    """``cost`` [L, R, T] -> ``(rows [L, n], cols [L, n], status [2])`` as the operator returns them: a problem that is
    INVALID counts in status[0], one that is INFEASIBLE in status[1], and either gets the filler pairs (k, k)."""
    c = np.asarray(cost)
    L, R, T = c.shape
    n = min(R, T)
    rows, cols, status = np.zeros((L, n), np.int64), np.zeros((L, n), np.int64), np.zeros(2, np.int32)
    for l in range(L):
        res = solve(c[l])
        if isinstance(res, str):
            status[0 if res == INVALID else 1] += 1
            res = (np.arange(n), np.arange(n))
        rows[l], cols[l] = res
    return rows, cols, status


def rank_one(n, m, seed):
    """The worst case of the method: ``-outer(a, b)`` with ``a`` and ``b`` sorted uniform float32.  Every augmentation walks
    the whole matching made so far, n(n+1)/2 steps in all."""
    rng = np.random.RandomState(seed)
    a, b = np.sort(rng.rand(n).astype(np.float32)), np.sort(rng.rand(m).astype(np.float32))
    return -np.outer(a, b).astype(np.float32)
