/*
 * assign.h -- C ABI of the linear sum assignment solver in libmsda_hip.so: what the Hungarian
 * matchers of DeVIS do with the cost matrix of boxmatch_cost (scipy.optimize.linear_sum_assignment), on the device, so that a
 * matcher call needs no device-to-host transfer.
 *
 * Problem.  cost [L, R, T], dense, float32 (ASSIGN_F32) or float64 (ASSIGN_F64): L independent problems.  With n = min(R, T)
 * a problem's result is n pairs (row, col), no row and no column twice, of the lowest total cost[row, col]; rows and cols are
 * int64 [L, n], the pairs of a problem ordered by ascending row (what scipy returns for both orientations).
 *
 * Algorithm: the shortest-augmenting-path method of Crouse 2016, the one scipy documents.  All arithmetic is double whatever
 * `dtype` is (a float32 entry converts exactly).  With R > T the problem is solved transposed: the shorter side (n) is
 * augmented one row at a time, the longer side (m columns) is scanned.  A step relaxes every unscanned column j from the
 * current row i with the reduced cost
 *     minv + c[i, j] - u[i] - v[j]            evaluated left to right (nothing is multiplied: no contraction is possible)
 * and scans the unscanned column of the lowest shortest-path value.  Ties break first in favour of a column that has no row
 * yet, then in favour of the lowest column index.  The rule is part of the contract: tests/assign_oracle.py states the same
 * algorithm in numpy, and the results agree bit for bit also where the optimum is not unique.  Where it is unique they are
 * scipy's.
 *
 * status int32 [2], zeroed by the call on `stream` and then counted with integer atomic adds, each problem at most once:
 *     [0] problems holding a NaN or a -inf entry (scipy: "matrix contains invalid numeric entries");
 *     [1] problems that +inf entries make infeasible (scipy: "cost matrix is infeasible").
 *   A feasible problem with +inf entries is solved normally.  A counted problem gets the in-range filler pairs (k, k), k < n,
 *   so that nothing downstream can index out of bounds; status is how the caller learns of it.  The other problems of the
 *   call are unaffected: a problem has the same result alone and among others, and every result is bitwise reproducible.
 *   L * n == 0 is a no-op that dereferences and writes nothing, status included.
 *
 * Termination does not depend on the data: every loop of the kernel is counted, with a bound taken from the shape -- n
 * augmentations, at most k + 1 steps in the k-th (at most n(n+1)/2 steps in all), at most k + 1 hops back along the path.
 * The NaN / -inf scan happens up front, and a step that finds no finite candidate ends its problem as infeasible.
 *
 * Limits: max(R, T) <= ASSIGN_MAX_SIDE (one 64-lane wave per problem holds the scanned side in registers), and L * R * T
 * fits 31 bits.
 *
 * Conventions (those of boxmatch.h)
 *   - every pointer is a DEVICE pointer; tensors are dense and need element alignment only;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and never
 *     synchronise (HIP-graph capture works), and are re-entrant;
 *   - element offsets are 64-bit;
 *   - return value: ASSIGN_OK (0) or a negative assign_status; on failure assign_last_error() returns a thread-local
 *     message.  Arguments are checked before any HIP call, so argument errors are reported without a GPU.
 */
#ifndef ASSIGN_H
#define ASSIGN_H

#ifdef __cplusplus
extern "C" {
#endif

#define ASSIGN_ABI_VERSION 1
#define ASSIGN_MAX_SIDE 1024

typedef enum assign_status { ASSIGN_OK = 0, ASSIGN_ERR_ARGUMENT = -1, ASSIGN_ERR_HIP = -2 } assign_status;

typedef enum assign_dtype { ASSIGN_F32 = 0, ASSIGN_F64 = 1 } assign_dtype;

int assign_version(void);
const char *assign_last_error(void);

int assign_solve(int dtype, const void *cost, int L, int R, int T, long long *rows, long long *cols, int *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ASSIGN_H */
