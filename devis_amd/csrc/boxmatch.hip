// boxmatch.hip -- the criterion's box geometry (include/boxmatch.h): the cost matrix of the Hungarian
// matchers and the two box losses of matched pairs, forward and backward, on one definition of the generalized IoU of two
// cxcywh boxes and of its derivative.  gfx950, wave64, plain HIP.  The workload is a few thousand results: every kernel is
// one launch of one lane per result with no workspace and no LDS, bound by launch latency, not tiled for a size it never has.
//
// The kernels are templates of the storage type of the predictions and of the targets (the same, or float beside 16 bits).
#include "op_common.h"       // (fp contraction off)
#include "boxmatch.h"

namespace boxmatch {

using namespace devis;

static_assert(BOXMATCH_OK == kOk && BOXMATCH_ERR_ARGUMENT == kErrArgument && BOXMATCH_ERR_HIP == kErrHip, "status codes");
static_assert(BOXMATCH_F32 == kF32 && BOXMATCH_F64 == kF64 && BOXMATCH_BF16 == kBF16 && BOXMATCH_F16 == kF16, "dtype codes");

constexpr int kThreads = 256;

thread_local Status err;     // boxmatch_last_error()

__device__ __forceinline__ float log_of(float v) { return logf(v); }
__device__ __forceinline__ double log_of(double v) { return log(v); }

template <typename A> __device__ __forceinline__ A sigmoid_of(A x)
{
    const A e = exp_of(-(x < (A)0 ? -x : x));
    const A inv = (A)1 / ((A)1 + e);
    return x >= (A)0 ? inv : e * inv;
}

// the focal cost of one logit (include/boxmatch.h cls): gamma is 2, 1 - p is sigmoid(-x)
template <typename A> __device__ __forceinline__ A class_cost_of(A x, A alpha)
{
    const A p = sigmoid_of(x), q = sigmoid_of(-x);
    const A pos = alpha * (q * q) * (-log_of(p + (A)1e-8));
    const A neg = ((A)1 - alpha) * (p * p) * (-log_of(q + (A)1e-8));
    return pos - neg;
}

template <typename A, typename T> __device__ __forceinline__ void load_box(const T *p, A b[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = (A)to_acc(p[k]);
}

// the sum over the 4 coordinates of |b - g|, in ascending order
template <typename A> __device__ __forceinline__ A l1_of(const A b[4], const A g[4])
{
    A sum = (A)0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const A d = b[k] - g[k];
        sum += d < (A)0 ? -d : d;
    }
    return sum;
}

// x1 < x0 or y1 < y0 after the conversion to corners (what the reference asserts on); false for NaN
template <typename A> __device__ __forceinline__ bool degenerate(const A b[4])
{
    const A h = (A)0.5;
    return b[0] + h * b[2] < b[0] - h * b[2] || b[1] + h * b[3] < b[1] - h * b[3];
}

// torch's max / min of two tensors and clamp(min=0); NaN goes through (a comparison with it is false)
template <typename A> __device__ __forceinline__ A hi_of(A a, A b) { return a != a ? a : (b > a || b != b ? b : a); }
template <typename A> __device__ __forceinline__ A lo_of(A a, A b) { return a != a ? a : (b < a || b != b ? b : a); }
template <typename A> __device__ __forceinline__ A clamp0(A v) { return v < (A)0 ? (A)0 : v; }
// the share of the gradient of max(a, b) / min(a, b) that goes to a: all, half on a tie, none
template <typename A> __device__ __forceinline__ A share_hi(A a, A b) { return a > b ? (A)1 : (a == b ? (A)0.5 : (A)0); }
template <typename A> __device__ __forceinline__ A share_lo(A a, A b) { return a < b ? (A)1 : (a == b ? (A)0.5 : (A)0); }
template <typename A> __device__ __forceinline__ A pass0(A v, A g) { return v >= (A)0 ? g : (A)0; }      // of clamp0

// THE definition of the generalized IoU of two cxcywh boxes (include/boxmatch.h): the value, and with kGrad its derivative
// with respect to s in d[4] (cx, cy, w, h), which is torch autograd's at the ties and at the clamps.
template <typename A, bool kGrad> __device__ __forceinline__ A giou_of(const A s[4], const A t[4], A d[4])
{
    const A h = (A)0.5, eps = (A)1e-6;
    const A sx0 = s[0] - h * s[2], sy0 = s[1] - h * s[3], sx1 = s[0] + h * s[2], sy1 = s[1] + h * s[3];
    const A tx0 = t[0] - h * t[2], ty0 = t[1] - h * t[3], tx1 = t[0] + h * t[2], ty1 = t[1] + h * t[3];
    const A sw = sx1 - sx0, sh = sy1 - sy0;
    const A area_s = sw * sh, area_t = (tx1 - tx0) * (ty1 - ty0);
    const A vw = lo_of(sx1, tx1) - hi_of(sx0, tx0), vh = lo_of(sy1, ty1) - hi_of(sy0, ty0);     // before the clamp
    const A iw = clamp0(vw), ih = clamp0(vh);
    const A inter = iw * ih;
    const A uni = area_s + area_t - inter;
    const A uw = hi_of(sx1, tx1) - lo_of(sx0, tx0), uh = hi_of(sy1, ty1) - lo_of(sy0, ty0);
    const A ew = clamp0(uw), eh = clamp0(uh);
    const A area = ew * eh;
    const A n1 = inter + eps, d1 = uni + eps, n2 = (area - uni) + eps, d2 = area + eps;
    const A value = n1 / d1 - n2 / d2;
    if constexpr (kGrad) {
        const A g_uni = (A)1 / d2 - n1 / (d1 * d1);              // through both ratios
        const A g_inter = (A)1 / d1 - g_uni;                     // union = area_s + area_t - inter
        const A g_area = n2 / (d2 * d2) - (A)1 / d2;
        const A g_iw = pass0(vw, g_inter * ih), g_ih = pass0(vh, g_inter * iw);
        const A g_ew = pass0(uw, g_area * eh), g_eh = pass0(uh, g_area * ew);
        const A gx1 = g_iw * share_lo(sx1, tx1) + g_ew * share_hi(sx1, tx1) + g_uni * sh;
        const A gx0 = -(g_iw * share_hi(sx0, tx0)) - g_ew * share_lo(sx0, tx0) - g_uni * sh;
        const A gy1 = g_ih * share_lo(sy1, ty1) + g_eh * share_hi(sy1, ty1) + g_uni * sw;
        const A gy0 = -(g_ih * share_hi(sy0, ty0)) - g_eh * share_lo(sy0, ty0) - g_uni * sw;
        d[0] = gx0 + gx1;
        d[1] = gy0 + gy1;
        d[2] = h * (gx1 - gx0);
        d[3] = h * (gy1 - gy0);
    }
    return value;
}

// ---- the matching cost -------------------------------------------------------------------------------------------------
// Lane e = (l * R + r) * T + t.  The lanes of t == 0 count their row's degenerate boxes, those of (l, r) == (0, 0) their
// target's degenerate boxes and bad labels: each item once.
template <typename T, typename TB>
__global__ __launch_bounds__(kThreads) void cost_kernel(const T *__restrict__ logits, const T *__restrict__ boxes,
                                                        const long long *__restrict__ labels, const TB *__restrict__ tgt_boxes,
                                                        typename Acc<T>::type *__restrict__ cost, int *__restrict__ status,
                                                        const boxmatch_shape s, const typename Acc<T>::type w_class,
                                                        const typename Acc<T>::type w_bbox, const typename Acc<T>::type w_giou,
                                                        const int l1_sum, const typename Acc<T>::type alpha)
{
    typedef typename Acc<T>::type A;
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (long long)s.L * s.R * s.T) return;
    const int t = (int)(e % s.T);
    const long long lr = e / s.T;
    const int r = (int)(lr % s.R), l = (int)(lr / s.R);
    A cls = (A)0, l1 = (A)0, gsum = (A)0;
    int bad_pred = 0, bad_tgt = 0, bad_label = 0;
    for (int f = 0; f < s.F; ++f) {
        const long long row = ((long long)l * s.F + f) * s.R + r, tf = (long long)t * s.F + f;
        const long long label = labels[tf];
        if (label >= 0 && label < s.C) {
            cls += class_cost_of((A)to_acc(logits[row * s.C + label]), alpha);
        } else {
            cls = (A)NAN;
            ++bad_label;
        }
        A b[4], g[4];
        load_box<A>(boxes + row * 4, b);
        load_box<A>(tgt_boxes + tf * 4, g);
        bad_pred += degenerate(b) ? 1 : 0;
        bad_tgt += degenerate(g) ? 1 : 0;
        l1 += l1_of(b, g);
        gsum += giou_of<A, false>(b, g, nullptr);
    }
    const A frames = (A)s.F;
    const A l1_term = l1_sum ? l1 / frames : l1 / ((A)4 * frames);
    cost[e] = (w_class * (cls / frames) + w_bbox * l1_term) + w_giou * (-(gsum / frames));
    if (t == 0 && bad_pred) atomicAdd(status + 0, bad_pred);
    if (lr == 0) {
        if (bad_tgt) atomicAdd(status + 1, bad_tgt);
        if (bad_label) atomicAdd(status + 2, bad_label);
    }
}

// ---- the box losses ------------------------------------------------------------------------------------------------------
template <typename T, typename TB>
__global__ __launch_bounds__(kThreads) void loss_forward_kernel(const T *__restrict__ src, const TB *__restrict__ tgt,
                                                                typename Acc<T>::type *__restrict__ l1,
                                                                typename Acc<T>::type *__restrict__ giou, const int N)
{
    typedef typename Acc<T>::type A;
    const long long n = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    A b[4], g[4];
    load_box<A>(src + n * 4, b);
    load_box<A>(tgt + n * 4, g);
    l1[n] = l1_of(b, g);
    giou[n] = (A)1 - giou_of<A, false>(b, g, nullptr);
}

template <typename T, typename TB>
__global__ __launch_bounds__(kThreads) void loss_backward_kernel(const T *__restrict__ src, const TB *__restrict__ tgt,
                                                                 const typename Acc<T>::type *__restrict__ grad_l1,
                                                                 const typename Acc<T>::type *__restrict__ grad_giou,
                                                                 T *__restrict__ grad_src, const int N)
{
    typedef typename Acc<T>::type A;
    const long long n = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    A b[4], g[4], d[4];
    load_box<A>(src + n * 4, b);
    load_box<A>(tgt + n * 4, g);
    giou_of<A, true>(b, g, d);
    const A gl = grad_l1[n], gg = grad_giou[n];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const A diff = b[k] - g[k];
        const A sign = diff > (A)0 ? (A)1 : (diff < (A)0 ? (A)-1 : (diff == (A)0 ? (A)0 : diff));     // (NaN stays NaN)
        from_acc(grad_src[n * 4 + k], gl * sign - gg * d[k]);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------
int check_codes(int dtype, int target)
{
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (target != BOXMATCH_TARGET_SAME && target != BOXMATCH_TARGET_F32) return err.fail("bad target kind %lld", target);
    if (target == BOXMATCH_TARGET_F32 && dtype == kF64)
        return err.fail("bad target kind %lld: float32 targets go with float32 or 16-bit predictions", target);
    return BOXMATCH_OK;
}

int check_rows(int N)
{
    if (N < 0) return err.fail("N must not be negative, got %lld", N);
    return BOXMATCH_OK;
}

}  // namespace boxmatch

using namespace boxmatch;

extern "C" {

int boxmatch_version(void) { return BOXMATCH_ABI_VERSION; }

const char *boxmatch_last_error(void) { return err.msg; }

int boxmatch_cost(int dtype, int target, const void *logits, const void *boxes, const long long *tgt_labels,
                  const void *tgt_boxes, const boxmatch_shape *shape, double cost_class, double cost_bbox, double cost_giou,
                  int l1, double alpha, void *cost, int *status, void *stream)
{
    err.clear();
    if (check_codes(dtype, target) != BOXMATCH_OK) return BOXMATCH_ERR_ARGUMENT;
    if (l1 != BOXMATCH_L1_MEAN && l1 != BOXMATCH_L1_SUM) return err.fail("bad l1 code %lld", l1);
    if (!shape) return err.fail("null pointer: shape");
    const boxmatch_shape &s = *shape;
    if (s.L < 0 || s.R < 0 || s.T < 0) return err.fail("L, R and T must not be negative");
    if (s.F <= 0 || s.C <= 0) return err.fail("F and C must be positive, got %lld and %lld", s.F, s.C);
    if (!(cost_class == cost_class) || !(cost_bbox == cost_bbox) || !(cost_giou == cost_giou) || !(alpha == alpha))
        return err.fail("the cost weights and alpha must not be NaN");
    const long long entries = (long long)s.L * s.R * s.T;
    if (entries > 0x7fffffffLL) return err.fail("L * R * T = %lld does not fit 31 bits", entries);
    if ((long long)s.L * s.F * s.R > 0x7fffffffLL) return err.fail("L * F * R = %lld does not fit 31 bits", (long long)s.L * s.F * s.R);
    if ((long long)s.T * s.F > 0x7fffffffLL) return err.fail("T * F = %lld does not fit 31 bits", (long long)s.T * s.F);
    if (entries == 0) return BOXMATCH_OK;
    if (!logits || !boxes || !tgt_labels || !tgt_boxes || !cost || !status)
        return err.fail("null pointer: logits, boxes, tgt_labels, tgt_boxes, cost and status are required");
    hipStream_t st = (hipStream_t)stream;
    unsigned grid;
    if (err.grid_of(cdiv(entries, kThreads), &grid)) return BOXMATCH_ERR_ARGUMENT;
    const hipError_t e = hipMemsetAsync(status, 0, 3 * sizeof(int), st);
    if (e != hipSuccess) return err.fail_hip("boxmatch_cost (zeroing status)", e);
    return dispatch(dtype, target == BOXMATCH_TARGET_F32, [&](auto t, auto tb) {
        typedef type_of<decltype(t)> T;
        typedef type_of<decltype(tb)> TB;
        typedef typename Acc<T>::type A;
        hipLaunchKernelGGL((cost_kernel<T, TB>), dim3(grid), dim3(kThreads), 0, st, (const T *)logits, (const T *)boxes, tgt_labels,
                           (const TB *)tgt_boxes, (A *)cost, status, s, (A)cost_class, (A)cost_bbox, (A)cost_giou,
                           l1 == BOXMATCH_L1_SUM ? 1 : 0, (A)alpha);
        return err.check_launch("boxmatch_cost");
    });
}

int boxmatch_loss_forward(int dtype, int target, const void *src, const void *tgt, int N, void *l1, void *giou, void *stream)
{
    err.clear();
    if (check_codes(dtype, target) != BOXMATCH_OK || check_rows(N) != BOXMATCH_OK) return BOXMATCH_ERR_ARGUMENT;
    if (N == 0) return BOXMATCH_OK;
    if (!src || !tgt || !l1 || !giou) return err.fail("null pointer: src, tgt, l1 and giou are required");
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)cdiv(N, kThreads);
    return dispatch(dtype, target == BOXMATCH_TARGET_F32, [&](auto t, auto tb) {
        typedef type_of<decltype(t)> T;
        typedef type_of<decltype(tb)> TB;
        typedef typename Acc<T>::type A;
        hipLaunchKernelGGL((loss_forward_kernel<T, TB>), dim3(grid), dim3(kThreads), 0, st, (const T *)src, (const TB *)tgt, (A *)l1,
                           (A *)giou, N);
        return err.check_launch("boxmatch_loss_forward");
    });
}

int boxmatch_loss_backward(int dtype, int target, const void *src, const void *tgt, const void *grad_l1, const void *grad_giou,
                           int N, void *grad_src, void *stream)
{
    err.clear();
    if (check_codes(dtype, target) != BOXMATCH_OK || check_rows(N) != BOXMATCH_OK) return BOXMATCH_ERR_ARGUMENT;
    if (N == 0) return BOXMATCH_OK;
    if (!src || !tgt || !grad_l1 || !grad_giou || !grad_src)
        return err.fail("null pointer: src, tgt, grad_l1, grad_giou and grad_src are required");
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)cdiv(N, kThreads);
    return dispatch(dtype, target == BOXMATCH_TARGET_F32, [&](auto t, auto tb) {
        typedef type_of<decltype(t)> T;
        typedef type_of<decltype(tb)> TB;
        typedef typename Acc<T>::type A;
        hipLaunchKernelGGL((loss_backward_kernel<T, TB>), dim3(grid), dim3(kThreads), 0, st, (const T *)src, (const TB *)tgt,
                           (const A *)grad_l1, (const A *)grad_giou, (T *)grad_src, N);
        return err.check_launch("boxmatch_loss_backward");
    });
}

}  // extern "C"
