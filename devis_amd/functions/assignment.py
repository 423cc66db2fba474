"""Host side of the linear sum assignment solver (include/assign.h): argument checks, the output tensors
and the one kernel launch.  The custom op of :mod:`devis_amd.ops` runs exactly this code.

The kernel is one wave per problem with every loop counted and no floating-point atomics: the indices are bitwise
reproducible, and a problem has the same result alone and among others.

There is no CPU path and no eager fallback: CPU tensors raise, a failing kernel call raises.
"""
import torch

from .. import _assign
from ._common import _check_device, _require

MAX_SIDE = _assign.MAX_SIDE


def check_cost(cost):
    """Shape and dtype contract of linear_assignment; raises before anything is launched.  Works on fake tensors.  Returns
    (L, R, T)."""
    _require(cost.dim() == 3, "linear_assignment: cost must be [L, R, T]")
    _require(cost.dtype in _assign.DTYPE_CODES,
             "linear_assignment: cost must be float32 or float64 (what match_cost returns), got %s" % (cost.dtype,))
    L, R, T = cost.shape
    _require(R <= MAX_SIDE and T <= MAX_SIDE,
             "linear_assignment: a problem of %s x %s exceeds the limit of %d on a side" % (R, T, MAX_SIDE))
    return L, R, T


def fits(R, T):
    """Whether an R x T problem is within the operator's limits (decided from the shape alone)."""
    return R <= MAX_SIDE and T <= MAX_SIDE


def _solve(cost):
    """(rows int64 [L, n], cols int64 [L, n], status int32 [2]), n = min(R, T)."""
    L, R, T = check_cost(cost)
    _check_device("linear_assignment", [("cost", cost)])
    n = min(R, T)
    rows = torch.empty((L, n), dtype=torch.int64, device=cost.device)
    cols = torch.empty((L, n), dtype=torch.int64, device=cost.device)
    if L * n == 0:
        return rows, cols, torch.zeros(2, dtype=torch.int32, device=cost.device)
    status = torch.empty(2, dtype=torch.int32, device=cost.device)          # (zeroed by the call)
    _assign.solve(_assign.DTYPE_CODES[cost.dtype], cost.contiguous(), L, R, T, rows, cols, status)
    return rows, cols, status
