// labelloss.hip -- the criterion's label loss (include/labelloss.h): the target class of every query
// from the matcher's indices, the sigmoid focal loss of all logits against them and the matched queries' top-1 count, forward
// and backward.  gfx950, wave64, plain HIP.  The workload is some ten thousand logits and at most a few hundred matches: the
// kernels are bound by launch latency, so the forward is one launch (two beyond one tile), the backward one, nothing is zeroed
// and there is no atomic on memory.
#include "op_common.h"       // (fp contraction off)
#include "labelloss.h"

namespace labelloss {

using namespace devis;

static_assert(LABELLOSS_OK == kOk && LABELLOSS_ERR_ARGUMENT == kErrArgument && LABELLOSS_ERR_HIP == kErrHip, "status codes");
static_assert(LABELLOSS_F32 == kF32 && LABELLOSS_F64 == kF64 && LABELLOSS_BF16 == kBF16 && LABELLOSS_F16 == kF16, "dtype codes");

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 4096;                 // logits per forward workgroup, whole rows: also the most rows a tile can have
constexpr int kRecord = 32;                 // bytes of a tile's record: the focal partial at 0, the four counts at 8
constexpr int kNoIndex = 0x7fffffff;

thread_local Status err;     // labelloss_last_error()

// ---- one element (include/labelloss.h) ---------------------------------------------------------------------------------
template <typename A> struct Element {
    A p, q, ce, m;      // sigmoid(x), sigmoid(-x), cross entropy, 1 - p_t
};

template <typename A> __device__ __forceinline__ Element<A> element_of(A x, bool t)
{
    Element<A> v;
    const A e = exp_of(-(x < (A)0 ? -x : x));
    const A inv = (A)1 / ((A)1 + e);
    v.p = x >= (A)0 ? inv : e * inv;
    v.q = x >= (A)0 ? e * inv : inv;
    const A z = t ? -x : x;                                 // max(x, 0) - x * t is max(-x, 0) for t = 1
    v.ce = (z > (A)0 ? z : (A)0) + log1p_of(e);             // (a NaN comes back through e)
    v.m = t ? v.q : v.p;
    return v;
}

template <typename A> __device__ __forceinline__ A alpha_of(bool t, A alpha)
{
    return alpha >= (A)0 ? (t ? alpha : (A)1 - alpha) : (A)1;
}

template <typename A> __device__ __forceinline__ A focal_of(A x, bool t, A alpha)
{
    const Element<A> v = element_of(x, t);
    return v.ce * v.m * v.m * alpha_of(t, alpha);
}

template <typename A> __device__ __forceinline__ A dfocal_of(A x, bool t, A alpha)
{
    const Element<A> v = element_of(x, t);
    const A diff = t ? -v.q : v.p, sign = t ? (A)-1 : (A)1;        // p - t without the cancellation, and 1 - 2t
    return alpha_of(t, alpha) * (diff * (v.m * v.m) + v.ce * ((A)2 * v.m) * sign * (v.p * v.q));
}

__device__ __forceinline__ bool is_valid(const unsigned char *valid, int m) { return !valid || valid[m] != 0; }

// ---- forward ------------------------------------------------------------------------------------------------------------
// Workgroup `tile` owns the rows [tile * rpt, tile * rpt + nrows) and their nrows * C consecutive logits.  tiles == 1: the
// call's results; otherwise the tile's record -> ws + tile * kRecord.
template <typename T>
__global__ __launch_bounds__(kThreads) void forward_kernel(const T *__restrict__ logits, const long long *__restrict__ rows,
                                                           const long long *__restrict__ labels,
                                                           const unsigned char *__restrict__ valid, int *__restrict__ target_classes,
                                                           unsigned char *__restrict__ ws,
                                                           typename Acc<T>::type *__restrict__ focal_sum, int *__restrict__ counts,
                                                           const labelloss_shape s, const int rpt, const int tiles,
                                                           const typename Acc<T>::type alpha)
{
    typedef typename Acc<T>::type A;
    __shared__ int table[kTile];            // per row: the highest good m, then the target class
    __shared__ A red[kWaves];
    __shared__ int cnt[4][kWaves];
    const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = tile * rpt;
    const int nrows = s.R - row0 < rpt ? s.R - row0 : rpt;
    for (int i = tid; i < nrows; i += kThreads) table[i] = -1;
    __syncthreads();
    int bad_rows = 0, bad_labels = 0;
    for (int m = tid; m < s.M; m += kThreads) {
        if (!is_valid(valid, m)) continue;
        const long long r = rows[m], l = labels[m];
        const bool row_ok = r >= 0 && r < s.R, label_ok = l >= 0 && l <= s.C;
        bad_rows += row_ok ? 0 : 1;
        bad_labels += label_ok ? 0 : 1;
        if (row_ok && label_ok && r >= row0 && r < (long long)row0 + nrows) atomicMax(&table[(int)(r - row0)], m);
    }
    __syncthreads();
    for (int i = tid; i < nrows; i += kThreads) {
        const int m = table[i];
        const int cls = m >= 0 ? (int)labels[m] : s.C;
        target_classes[row0 + i] = cls;
        table[i] = cls;
    }
    __syncthreads();
    // the focal terms: a lane's elements ascending
    const long long base = (long long)row0 * s.C, count = (long long)nrows * s.C;
    A acc = (A)0;
    for (long long e = tid; e < count; e += kThreads) {
        const int i = (int)(e / s.C), c = (int)(e - (long long)i * s.C);
        acc += focal_of((A)to_acc(logits[base + e]), c == table[i], alpha);
    }
    acc = wave_sum(acc);
    // the argmax of every good match of these rows: one wave per match, the lowest index on ties, none with a NaN
    int good = 0, correct = 0;
    for (int m = wave; m < s.M; m += kWaves) {
        if (!is_valid(valid, m)) continue;
        const long long r = rows[m], l = labels[m];
        if (!(r >= row0 && r < (long long)row0 + nrows && l >= 0 && l <= s.C)) continue;
        const T *row = logits + r * s.C;
        A best = neg_inf((A)0);
        int at = kNoIndex, nan = 0;
        for (int c = lane; c < s.C; c += 64) {
            const A v = (A)to_acc(row[c]);
            nan |= v != v ? 1 : 0;
            if (v > best || (v == best && c < at)) {
                best = v;
                at = c;
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const A ob = __shfl_xor(best, d, 64);
            const int oa = __shfl_xor(at, d, 64);
            nan |= __shfl_xor(nan, d, 64);
            if (ob > best || (ob == best && oa < at)) {
                best = ob;
                at = oa;
            }
        }
        good += 1;
        correct += !nan && (long long)at == l ? 1 : 0;
    }
    bad_rows = wave_sum(bad_rows);
    bad_labels = wave_sum(bad_labels);
    if (lane == 0) {
        red[wave] = acc;
        cnt[0][wave] = good; cnt[1][wave] = correct; cnt[2][wave] = bad_rows; cnt[3][wave] = bad_labels;
    }
    __syncthreads();
    if (tid == 0) {
        A f = red[0];
        int n[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) n[k] = cnt[k][0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            f += red[w];
#pragma unroll
            for (int k = 0; k < 4; ++k) n[k] += cnt[k][w];
        }
        if (tile != 0) n[2] = n[3] = 0;         // (every workgroup sees every match: workgroup 0 counts the bad ones)
        A *fdst = tiles == 1 ? focal_sum : reinterpret_cast<A *>(ws + (long long)tile * kRecord);
        int *ndst = tiles == 1 ? counts : reinterpret_cast<int *>(ws + (long long)tile * kRecord + 8);
        *fdst = f;
#pragma unroll
        for (int k = 0; k < 4; ++k) ndst[k] = n[k];
    }
}

// One workgroup: lanes strided over the records ascending, butterflies, waves ascending.
template <typename A>
__global__ __launch_bounds__(kThreads) void combine_kernel(const unsigned char *__restrict__ ws, A *__restrict__ focal_sum,
                                                           int *__restrict__ counts, const int tiles)
{
    __shared__ A red[kWaves];
    __shared__ int cnt[4][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    A f = (A)0;
    int n[4] = {0, 0, 0, 0};
    for (int i = tid; i < tiles; i += kThreads) {
        f += *reinterpret_cast<const A *>(ws + (long long)i * kRecord);
        const int *src = reinterpret_cast<const int *>(ws + (long long)i * kRecord + 8);
#pragma unroll
        for (int k = 0; k < 4; ++k) n[k] += src[k];
    }
    f = wave_sum(f);
#pragma unroll
    for (int k = 0; k < 4; ++k) n[k] = wave_sum(n[k]);
    if (lane == 0) {
        red[wave] = f;
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt[k][wave] = n[k];
    }
    __syncthreads();
    if (tid == 0) {
        A total = red[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) total += red[w];
        *focal_sum = total;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int v = cnt[k][0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) v += cnt[k][w];
            counts[k] = v;
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void backward_kernel(const T *__restrict__ logits, const int *__restrict__ target_classes,
                                                            const typename Acc<T>::type *__restrict__ grad_sum,
                                                            T *__restrict__ grad_logits, const int C, const long long total,
                                                            const typename Acc<T>::type alpha)
{
    typedef typename Acc<T>::type A;
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= total) return;
    const long long r = e / C;
    const int c = (int)(e - r * C);
    const A g = grad_sum[0];
    from_acc(grad_logits[e], g * dfocal_of((A)to_acc(logits[e]), c == target_classes[r], alpha));
}

// ---- host -----------------------------------------------------------------------------------------------------------
int check_shape(const labelloss_shape *s)
{
    if (!s) return err.fail("null pointer: shape");
    if (s->R < 0 || s->C < 0 || s->M < 0) return err.fail("R, C and M must not be negative");
    if ((long long)s->R * s->C > 0x7fffffffLL) return err.fail("R * C = %lld does not fit 31 bits", (long long)s->R * s->C);
    return LABELLOSS_OK;
}

int rows_per_tile(const labelloss_shape &s) { return s.C >= kTile ? 1 : kTile / s.C; }       // (C > 0)
int tiles_of(const labelloss_shape &s) { return (int)cdiv(s.R, rows_per_tile(s)); }

}  // namespace labelloss

using namespace labelloss;

extern "C" {

int labelloss_version(void) { return LABELLOSS_ABI_VERSION; }

const char *labelloss_last_error(void) { return err.msg; }

int labelloss_tile(int which)
{
    switch (which) {
    case LABELLOSS_TILE_ELEMENTS: return kTile;
    default: return -1;
    }
}

long long labelloss_workspace_bytes(int dtype, const labelloss_shape *shape)
{
    err.clear();
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (check_shape(shape) != LABELLOSS_OK) return LABELLOSS_ERR_ARGUMENT;
    if ((long long)shape->R * shape->C == 0) return 0;
    const int tiles = tiles_of(*shape);
    const long long bytes = tiles > 1 ? (long long)tiles * kRecord : 0;
    return (bytes + 255) / 256 * 256;
}

int labelloss_forward(int dtype, const void *logits, const long long *rows, const long long *labels,
                      const unsigned char *valid, const labelloss_shape *shape, double alpha, void *workspace,
                      int *target_classes, void *focal_sum, int *counts, void *stream)
{
    err.clear();
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (check_shape(shape) != LABELLOSS_OK) return LABELLOSS_ERR_ARGUMENT;
    if (!(alpha == alpha)) return err.fail("alpha must be a number");
    const labelloss_shape &s = *shape;
    if ((long long)s.R * s.C == 0) return LABELLOSS_OK;
    if (!logits || !target_classes || !focal_sum || !counts)
        return err.fail("null pointer: logits, target_classes, focal_sum and counts are required");
    if (s.M > 0 && (!rows || !labels)) return err.fail("null pointer: rows and labels are required when there are matches");
    const int rpt = rows_per_tile(s), tiles = tiles_of(s);
    if (!workspace && tiles > 1) return err.fail("null pointer: workspace is required when the call is more than one tile");
    hipStream_t st = (hipStream_t)stream;
    return dispatch(dtype, [&](auto t) {
        typedef type_of<decltype(t)> T;
        typedef typename Acc<T>::type A;
        hipLaunchKernelGGL((forward_kernel<T>), dim3((unsigned)tiles), dim3(kThreads), 0, st, (const T *)logits, rows, labels, valid,
                           target_classes, (unsigned char *)workspace, (A *)focal_sum, counts, s, rpt, tiles, (A)alpha);
        if (tiles > 1)
            hipLaunchKernelGGL((combine_kernel<A>), dim3(1), dim3(kThreads), 0, st, (const unsigned char *)workspace,
                               (A *)focal_sum, counts, tiles);
        return err.check_launch("labelloss_forward");
    });
}

int labelloss_backward(int dtype, const void *logits, const int *target_classes, const void *grad_sum,
                       const labelloss_shape *shape, double alpha, void *grad_logits, void *stream)
{
    err.clear();
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (check_shape(shape) != LABELLOSS_OK) return LABELLOSS_ERR_ARGUMENT;
    if (!(alpha == alpha)) return err.fail("alpha must be a number");
    const long long total = (long long)shape->R * shape->C;
    if (total == 0) return LABELLOSS_OK;
    if (!logits || !target_classes || !grad_sum || !grad_logits)
        return err.fail("null pointer: logits, target_classes, grad_sum and grad_logits are required");
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)cdiv(total, kThreads);
    const int C = shape->C;
    return dispatch(dtype, [&](auto t) {
        typedef type_of<decltype(t)> T;
        typedef typename Acc<T>::type A;
        hipLaunchKernelGGL((backward_kernel<T>), dim3(grid), dim3(kThreads), 0, st, (const T *)logits, target_classes,
                           (const A *)grad_sum, (T *)grad_logits, C, total, (A)alpha);
        return err.check_launch("labelloss_backward");
    });
}

}  // extern "C"
