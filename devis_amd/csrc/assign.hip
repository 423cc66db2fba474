// assign.hip -- the linear sum assignment solver (include/assign.h): the shortest-augmenting-path
// method of Crouse 2016 with the tie rule the header states, one 64-lane wave per problem, grid = L.  gfx950, wave64, plain HIP.
//
// The scanned side (m = max(R, T) columns) is strided over the lanes: lane l holds columns l, l + 64, ... -- K = ceil(m / 64)
// of them, K a template parameter in {1, 2, 4, 8, 16} -- with their dual v, shortest-path value, predecessor and row in
// registers, indexed by unrolled loops only.  The augmented side (n = min(R, T) rows: the dual u and the column of a row) is
// indexed by data and lives in LDS.  A step is lane-local work and one 64-lane argmin: DPP row operations and ballots.  There is no barrier and
// no inter-wave traffic: the one wave orders its own LDS accesses with a wavefront-scope fence.  Every loop is counted.
#include "op_common.h"       // (fp contraction off)
#include "assign.h"

namespace assign {

using namespace devis;

static_assert(ASSIGN_OK == kOk && ASSIGN_ERR_ARGUMENT == kErrArgument && ASSIGN_ERR_HIP == kErrHip, "status codes");
static_assert(ASSIGN_F32 == kF32 && ASSIGN_F64 == kF64, "dtype codes");
static_assert(ASSIGN_MAX_SIDE == 64 * 16, "the largest K covers ASSIGN_MAX_SIDE columns");

constexpr int kLanes = 64;
constexpr int kStageBytes = 48 << 10;    // a cost block of at most this many bytes is staged in LDS (beside 12 KiB of row state)
constexpr int kNoCandidate = 0x7fffffff;

thread_local Status err;     // assign_last_error()

// A candidate of the argmin is (shortest-path value, key); key = has-row << 20 | column << 10 | row (0 without one), so that
// among equal values a column without a row comes first, then the lowest column.  Columns differ, so the order is total.
__device__ __forceinline__ bool before(double av, int ak, double bv, int bk) { return av < bv || (av == bv && ak < bk); }

// orders this wave's LDS accesses (one lane writes what another reads); no instruction of its own beyond a wait
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The lowest of a value over the 64 lanes, in every lane (as a scalar): quad permutes and row rotations (DPP) leave each row of
// 16 lanes with its lowest, and the four rows are read by lane.  No LDS traffic: this is the dependent step's critical path.
template <int kCtrl> __device__ __forceinline__ double dpp_of(double v)
{
    const int hi = __double2hiint(v), lo = __double2loint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, kCtrl, 0xf, 0xf, false),
                            __builtin_amdgcn_update_dpp(lo, lo, kCtrl, 0xf, 0xf, false));
}

__device__ __forceinline__ double lower_of(double a, double b) { return b < a ? b : a; }

__device__ __forceinline__ double value_of_lane(double v, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

__device__ __forceinline__ double wave_lowest(double v)
{
    v = lower_of(v, dpp_of<0xb1>(v));        // quad_perm [1, 0, 3, 2]
    v = lower_of(v, dpp_of<0x4e>(v));        // quad_perm [2, 3, 0, 1]
    v = lower_of(v, dpp_of<0x124>(v));       // row_ror 4
    v = lower_of(v, dpp_of<0x128>(v));       // row_ror 8
    return lower_of(lower_of(value_of_lane(v, 15), value_of_lane(v, 31)), lower_of(value_of_lane(v, 47), value_of_lane(v, 63)));
}

__device__ __forceinline__ void fill_identity(long long *rows, long long *cols, int n, int lane)
{
    for (int k = lane; k < n; k += kLanes) rows[k] = cols[k] = k;
}

// Zeroes status ahead of the solver on the same stream.  A kernel, not hipMemsetAsync as in boxmatch.hip: replayed from a
// captured graph, the 8-byte memset node of this status was seen to write a stale byte value (the 12-byte one of
// boxmatch_cost replays correctly); a launch replays as what it is.
__global__ __launch_bounds__(kLanes) void zero_status_kernel(int *__restrict__ status)
{
    if (threadIdx.x < 2) status[threadIdx.x] = 0;
}

template <typename T, int K>
__global__ __launch_bounds__(kLanes) void solve_kernel(const T *__restrict__ cost, long long *__restrict__ rows,
                                                       long long *__restrict__ cols, int *__restrict__ status, const int R,
                                                       const int Tn, const int staged)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const double inf = (double)INFINITY;
    const int lane = threadIdx.x;
    const bool transposed = R > Tn;
    const int n = transposed ? Tn : R, m = transposed ? R : Tn;
    const int si = transposed ? 1 : Tn, sj = transposed ? Tn : 1;            // entry (i, j) of the solved problem is c[i * si + j * sj]
    const T *c = cost + (long long)blockIdx.x * R * Tn;
    long long *out_r = rows + (long long)blockIdx.x * n, *out_c = cols + (long long)blockIdx.x * n;
    double *u = (double *)lds;                                                // [n]
    T *block = (T *)(u + n);                                                  // [n, m] when staged
    int *col4row = (int *)(block + (staged ? n * m : 0));                     // [n]

    // up front: the NaN / -inf scan (and the staging, in the order of the memory)
    bool bad = false;
    for (int e = lane; e < n * m; e += kLanes) {
        const T x = c[e];
        bad |= x != x || x == -(T)INFINITY;
        if (staged) block[transposed ? (e % n) * m + e / n : e] = x;
    }
    for (int i = lane; i < n; i += kLanes) {
        u[i] = 0.0;
        col4row[i] = -1;
    }
    wave_sync();
    if (__any(bad)) {
        fill_identity(out_r, out_c, n, lane);
        if (lane == 0) atomicAdd(status + 0, 1);
        return;
    }

    double v[K], spc[K];
    int path[K], row4col[K];
    unsigned dead = 0;                       // bit k: column lane + 64 * k does not exist
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = 0.0;
        path[k] = 0;
        row4col[k] = -1;
        if (lane + kLanes * k >= m) dead |= 1u << k;
    }

    bool feasible = true;
    for (int cur = 0; cur < n && feasible; ++cur) {
        unsigned scanned = dead;
#pragma unroll
        for (int k = 0; k < K; ++k) spc[k] = inf;
        double minv = 0.0;
        int i = cur, sink = -1;
        for (int step = 0; step <= cur; ++step) {        // a step scans one column; all but the last hold one of the cur rows
            const double ui = u[i];
            double bv = inf;
            int bk = kNoCandidate;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (scanned >> k & 1) continue;
                const int j = lane + kLanes * k;
                const double cij = staged ? (double)block[i * m + j] : (double)c[i * si + j * sj];
                const double r = ((minv + cij) - ui) - v[k];
                if (r < spc[k]) {
                    spc[k] = r;
                    path[k] = i;
                }
                const int key = row4col[k] < 0 ? j << 10 : (1 << 20 | j << 10 | row4col[k]);
                if (before(spc[k], key, bv, bk)) {
                    bv = spc[k];
                    bk = key;
                }
            }
            // the wave's argmin: the lowest value first, then among the lanes that hold it the lowest key
            const double lowest = wave_lowest(bv);
            const bool holds = bv == lowest;
            const unsigned long long free_ones = __ballot(holds && !(bk >> 20));
            const unsigned long long pool = free_ones ? free_ones : __ballot(holds);
            const bool in_pool = pool >> lane & 1;
            int winner = 0;
#pragma unroll
            for (int k = K - 1; k >= 0; --k) {           // (a lane's column of slot k is lane + 64 * k: the lowest slot, then the lowest lane)
                const unsigned long long here = __ballot(in_pool && (bk >> 16 & 15) == k);
                winner = here ? __builtin_ctzll(here) : winner;
            }
            bv = lowest;
            bk = __builtin_amdgcn_readlane(bk, winner);
            if (!(bv < inf)) break;                      // no finite candidate: infeasible (sink stays -1)
            minv = bv;
            const int j = bk >> 10 & 1023;
            if ((j & 63) == lane) scanned |= 1u << (j >> 6);
            if (!(bk >> 20)) {
                sink = j;
                break;
            }
            i = bk & 1023;
        }
        if (sink < 0) {
            feasible = false;
            break;
        }
        // the dual update: every scanned column, and the row it holds (the sink's difference is 0 and it holds none)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (!((scanned & ~dead) >> k & 1)) continue;
            const double d = minv - spc[k];
            if (row4col[k] >= 0) u[row4col[k]] += d;
            v[k] -= d;
        }
        if (lane == 0) u[cur] += minv;
        wave_sync();
        // back along the path: at most cur + 1 columns
        int j = __builtin_amdgcn_readfirstlane(sink);
        for (int hop = 0; hop <= cur; ++hop) {
            const int kk = j >> 6, owner = j & 63;
            int p = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) p = k == kk ? path[k] : p;
            const int row = __builtin_amdgcn_readlane(p, owner);          // (j is the same in every lane)
#pragma unroll
            for (int k = 0; k < K; ++k) row4col[k] = (k == kk && lane == owner) ? row : row4col[k];
            const int prev = __builtin_amdgcn_readfirstlane(col4row[row]);
            if (lane == 0) col4row[row] = j;
            wave_sync();
            j = prev;
            if (row == cur || prev < 0) break;
        }
    }
    if (!feasible) {
        fill_identity(out_r, out_c, n, lane);
        if (lane == 0) atomicAdd(status + 1, 1);
        return;
    }
    // the pairs by ascending row
    if (!transposed) {
        for (int i = lane; i < n; i += kLanes) {
            out_r[i] = i;
            out_c[i] = col4row[i];
        }
    } else {                                 // a column of the solved problem is a row of the caller's: j ascends with k, then the lane
        int base = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool has = row4col[k] >= 0;
            const unsigned long long mask = __ballot(has);
            const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
            if (has && pos < n) {
                out_r[pos] = lane + kLanes * k;
                out_c[pos] = row4col[k];
            }
            base += __popcll(mask);
        }
    }
}

template <typename T, int K>
int launch(const void *cost, int L, int R, int Tn, long long *rows, long long *cols, int *status, hipStream_t st)
{
    const long long n = R < Tn ? R : Tn, m = R < Tn ? Tn : R;
    const int staged = n * m * (long long)sizeof(T) <= kStageBytes ? 1 : 0;
    const size_t bytes = (size_t)(n * 8 + (staged ? n * m * (long long)sizeof(T) : 0) + n * 4);
    hipLaunchKernelGGL((solve_kernel<T, K>), dim3((unsigned)L), dim3(kLanes), bytes, st, (const T *)cost, rows, cols, status, R,
                       Tn, staged);
    return err.check_launch("assign_solve");
}

template <typename T>
int launch_k(const void *cost, int L, int R, int Tn, long long *rows, long long *cols, int *status, hipStream_t st)
{
    const int m = R < Tn ? Tn : R;
    if (m <= 64) return launch<T, 1>(cost, L, R, Tn, rows, cols, status, st);
    if (m <= 128) return launch<T, 2>(cost, L, R, Tn, rows, cols, status, st);
    if (m <= 256) return launch<T, 4>(cost, L, R, Tn, rows, cols, status, st);
    if (m <= 512) return launch<T, 8>(cost, L, R, Tn, rows, cols, status, st);
    return launch<T, 16>(cost, L, R, Tn, rows, cols, status, st);
}

}  // namespace assign

using namespace assign;

extern "C" {

int assign_version(void) { return ASSIGN_ABI_VERSION; }

const char *assign_last_error(void) { return err.msg; }

int assign_solve(int dtype, const void *cost, int L, int R, int T, long long *rows, long long *cols, int *status, void *stream)
{
    err.clear();
    if (dtype != ASSIGN_F32 && dtype != ASSIGN_F64) return err.fail("bad dtype code %lld (float32 and float64 costs only)", dtype);
    if (L < 0 || R < 0 || T < 0) return err.fail("L, R and T must not be negative");
    if (R > ASSIGN_MAX_SIDE || T > ASSIGN_MAX_SIDE)
        return err.fail("a side of %lld exceeds the limit of %lld", R > T ? R : T, ASSIGN_MAX_SIDE);
    const long long entries = (long long)L * R * T;
    if (entries > 0x7fffffffLL) return err.fail("L * R * T = %lld does not fit 31 bits", entries);
    if (entries == 0) return ASSIGN_OK;          // (L * min(R, T) == 0)
    if (!cost || !rows || !cols || !status) return err.fail("null pointer: cost, rows, cols and status are required");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(zero_status_kernel, dim3(1), dim3(kLanes), 0, st, status);
    if (err.check_launch("assign_solve (zeroing status)") != ASSIGN_OK) return ASSIGN_ERR_HIP;
    return dtype == ASSIGN_F32 ? launch_k<float>(cost, L, R, T, rows, cols, status, st)
                               : launch_k<double>(cost, L, R, T, rows, cols, status, st);
}

}  // extern "C"
