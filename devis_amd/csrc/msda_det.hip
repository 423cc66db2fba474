// msda_det.hip -- grad_value whose every element depends only on the multiset of terms that reach it
// (include/msda.h, MSDA_GRAD_DETERMINISTIC): the backward under torch.use_deterministic_algorithms(True).
//
// Float sums depend on their order, integer sums do not.  Every term  w_corner * attn * grad_out[c]  (the reference's
// atomicAdd operand, ms_deform_im2col_cuda.cuh:125-152) is rounded to nearest-even onto a multiple of a quantum q = 2^e
// and added as int64; the result is acc * q, rounded once to the output type.  q is fixed per (clip, head) -- the value
// batch item whose pixels the terms reach -- from A = max |attn_weight| and G = max |grad_out| over that clip's finite
// values and n = its points per head (queries x points per query: a point's four corners land on four different pixels,
// so no pixel receives more than n terms): the smallest power of two with A * G * n <= 2^62 * q, so no sum overflows.
// Everything q depends on is the clip's own data, so a clip's gradient is the same alone or in a batch, in any query
// order, with any im2col_step.  Non-finite terms set bits of a per-element class nibble (NaN, +Inf, -Inf), combined by
// OR: the output is then what IEEE summation gives (NaN if any NaN or both infinities, else the infinity).
//
// Kernels, all on the stream of the call:
//   maxima    per (clip, head, part) workgroup, max of the finite |attn| and |grad_out| bits (unsigned order = magnitude
//             order for non-negative floats), one global_atomic_umax_x2 per wave: independent of order;
//   scatter   route (a), here: one lane per (row, point, channel), four int64 global atomic adds; any D and dtype, any level
//             layout, plain and temporal calls, levels of any width.  Route (b), msda_scatter.hip: the LDS-band scatter with
//             int64 band accumulators (ds_add_u64), for the fp32 / 16-bit calls it takes (D a multiple of 4).  Both form the
//             same terms (msda_det.h), so they give the same int64 sums and the same bits;
//   convert   every element of grad_value, gap rows included (they receive no terms: 0).
// Workspace (msda_backward_workspace_bytes_det): [clips * M * 2] u64 maxima, 256-B aligned, then [elems] int64
// accumulators, then [ceil(elems / 8)] u32 class words (4 bits per element); zeroed on the stream first.
#include "msda_common.h"
#include "msda_det.h"
#include "msda_plan.h"
#include <algorithm>

namespace msda {
namespace {

constexpr int kDetThreads = 256;

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
#pragma unroll
    for (int s = 1; s < kWave; s <<= 1) {
        const unsigned long long o = __shfl_xor(v, s, kWave);
        v = o > v ? o : v;
    }
    return v;
}

// grid (clips * M, parts): workgroup (clip, head) part `blockIdx.y` strides over that clip's attention weights (current
// and temporal) and grad_out rows of the head.
template <typename T, typename TL, typename A>
__global__ void __launch_bounds__(kDetThreads)
msda_det_maxima_kernel(const Params p, unsigned long long *maxima)
{
    const int item = blockIdx.x, m = item % p.M, clip = item / p.M;
    const int64_t rows = (int64_t)p.frames * p.Lq;                  // (frame, query) rows of the clip
    const int64_t row0 = (int64_t)clip * rows;
    const int64_t stride = (int64_t)gridDim.y * kDetThreads, start = (int64_t)blockIdx.y * kDetThreads + threadIdx.x;
    unsigned long long amax = 0, gmax = 0;
    for (int arr = 0; arr < 2; ++arr) {
        const TL *aw = static_cast<const TL *>(arr ? p.awB : p.awA);
        const int64_t K = arr ? (int64_t)p.LB * p.PB : (int64_t)p.LA * p.PA;
        if (!aw || K == 0) continue;
        for (int64_t j = start; j < rows * K; j += stride) {
            const int64_t r = j / K, k = j - r * K;
            const unsigned long long v = det_abs_bits<A>((A)Store<TL>::get(aw + ((row0 + r) * p.M + m) * K + k));
            amax = v > amax ? v : amax;
        }
    }
    const T *go = static_cast<const T *>(p.grad_out);
    for (int64_t j = start; j < rows * p.D; j += stride) {
        const int64_t r = j / p.D, c = j - r * p.D;
        const unsigned long long v = det_abs_bits<A>((A)Store<T>::get(go + ((row0 + r) * p.M + m) * p.D + c));
        gmax = v > gmax ? v : gmax;
    }
    amax = wave_max(amax);
    gmax = wave_max(gmax);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        atomicMax(maxima + 2 * item, amax);
        atomicMax(maxima + 2 * item + 1, gmax);
    }
}

// Taps of one sampling point with explicit round-to-nearest arithmetic (cuh:285-288 range test, cuh:38-80 corners):
// valid bit k set for corner k inside the map, pixel offsets relative to the clip slab.
template <typename A>
struct DetTaps { int64_t pix[4]; A w[4]; int valid; };

template <typename A>
__device__ __forceinline__ DetTaps<A> det_taps(A x, A y, const Level lv)
{
    using B = DetBits<A>;
    DetTaps<A> t;
    t.valid = 0;
    const A h_im = B::sub(B::mul(y, (A)lv.H), (A)0.5), w_im = B::sub(B::mul(x, (A)lv.W), (A)0.5);
    if (!(h_im > -1 && w_im > -1 && h_im < lv.H && w_im < lv.W)) return t;
    const A hf = floor(h_im), wf = floor(w_im);
    const int h_low = (int)hf, w_low = (int)wf;
    const A lh = B::sub(h_im, hf), lw = B::sub(w_im, wf), hh = B::sub((A)1, lh), hw = B::sub((A)1, lw);
    const bool y0 = h_low >= 0, y1 = h_low + 1 <= lv.H - 1, x0 = w_low >= 0, x1 = w_low + 1 <= lv.W - 1;
    const int64_t r0 = (int64_t)lv.start + (int64_t)h_low * lv.W + w_low;
    t.pix[0] = r0; t.pix[1] = r0 + 1; t.pix[2] = r0 + lv.W; t.pix[3] = r0 + lv.W + 1;
    t.w[0] = B::mul(hh, hw); t.w[1] = B::mul(hh, lw); t.w[2] = B::mul(lh, hw); t.w[3] = B::mul(lh, lw);
    t.valid = (y0 && x0 ? 1 : 0) | (y0 && x1 ? 2 : 0) | (y1 && x0 ? 4 : 0) | (y1 && x1 ? 8 : 0);
    return t;
}

// One lane per (row, point, channel), channel fastest: the four adds of a wave instruction are contiguous runs of D int64.
template <typename T, typename TL, typename A>
__global__ void __launch_bounds__(kDetThreads)
msda_det_scatter_kernel(const Params p, const DetArgs d, int64_t total)
{
    const int KA = p.LA * p.PA, KB = p.LB * p.PB, K = KA + KB;
    const long long n = det_terms_bound(p);
    const int64_t MD = (int64_t)p.M * p.D;
    for (int64_t i = (int64_t)blockIdx.x * kDetThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kDetThreads) {
        const int c = (int)(i % p.D);
        const int64_t rp = i / p.D;
        const int k = (int)(rp % K);
        const int64_t row = rp / K;                              // (group, query, head)
        const int m = (int)(row % p.M);
        const int group = (int)(row / ((int64_t)p.M * p.Lq));
        const int clip = group / p.frames, t = group - clip * p.frames;
        const bool temporal = k >= KA;
        const int kk = temporal ? k - KA : k, P = temporal ? p.PB : p.PA;
        const TL *loc = static_cast<const TL *>(temporal ? p.locB : p.locA);
        const TL *aw = static_cast<const TL *>(temporal ? p.awB : p.awA);
        const int64_t idx = row * (temporal ? KB : KA) + kk;
        const Level lv = make_level(p, t, (temporal ? p.LA : 0) + kk / P);
        const DetTaps<A> tp = det_taps<A>((A)Store<TL>::get(loc + 2 * idx), (A)Store<TL>::get(loc + 2 * idx + 1), lv);
        if (!tp.valid) continue;
        const A a = (A)Store<TL>::get(aw + idx);
        const A g = (A)Store<T>::get(static_cast<const T *>(p.grad_out) + row * p.D + c);
        const int e = det_exponent<A>(d.maxima + 2 * ((int64_t)clip * p.M + m), n);
        const int64_t base = (int64_t)clip * p.frames * p.S * MD + (int64_t)m * p.D + c;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (tp.valid & (1 << q)) det_add_global<A>(d, base + tp.pix[q] * MD, det_term<A>(det_weight<A>(tp.w[q], a), g), e);
    }
}

template <typename A, typename O>
__global__ void __launch_bounds__(kDetThreads)
msda_det_convert_kernel(const Params p, const unsigned long long *maxima, const long long *acc, const unsigned *cls,
                        O *out, int64_t total)
{
    const long long n = det_terms_bound(p);
    const int64_t clip_elems = (int64_t)p.frames * p.S * p.M * p.D;
    for (int64_t i = (int64_t)blockIdx.x * kDetThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kDetThreads) {
        const unsigned k = (cls[i >> 3] >> ((i & 7) * 4)) & 7u;
        A v;
        if ((k & 1) || (k & 6) == 6) {
            v = (A)NAN;
        } else if (k) {
            v = k == 2 ? (A)INFINITY : -(A)INFINITY;
        } else {
            const int64_t clip = i / clip_elems;
            const int m = (int)((i / p.D) % p.M);
            const int e = det_exponent<A>(maxima + 2 * (clip * p.M + m), n);
            v = DetBits<A>::ldexp_((A)acc[i], e);                   // one rounding (int64 -> A); the scaling is exact but at the range ends
        }
        Store<O>::put(out + i, v);
    }
}

unsigned det_blocks(int64_t work)
{
    const int64_t want = (work + kDetThreads - 1) / kDetThreads;
    return (unsigned)(want < 65536 * 16 ? want : 65536 * 16);
}

template <typename T, typename TL, typename A>
int det_prepare(const Params &p, char *ws, DetArgs &d, hipStream_t stream)
{
    const int64_t clips = p.groups / p.frames, items = clips * p.M;
    const int64_t elems = (int64_t)p.groups * p.S * p.M * p.D;
    unsigned long long *maxima = reinterpret_cast<unsigned long long *>(ws);
    d.maxima = maxima;
    d.acc = reinterpret_cast<long long *>(ws + plan::det_maxima_bytes(clips, p.M));
    d.cls = reinterpret_cast<unsigned *>(d.acc + elems);
    if (items > 0x7fffffffLL) return fail(MSDA_ERR_ARG, "msda: problem too large for one launch%s");
    if (hipMemsetAsync(ws, 0, (size_t)plan::det_workspace_bytes(clips, p.frames, p.S, p.M, p.D), stream) != hipSuccess)
        return fail(MSDA_ERR_HIP, "msda backward: hipMemsetAsync(deterministic workspace) failed%s");
    // (clip, head) workgroups, split so that a batch covers the chip about twice; a clip's maxima do not depend on the split
    const int64_t per_item = (int64_t)p.frames * p.Lq * std::max<int64_t>((int64_t)p.LA * p.PA + (int64_t)p.LB * p.PB, p.D);
    int64_t parts = std::min<int64_t>((per_item + 4 * kDetThreads - 1) / (4 * kDetThreads), std::max<int64_t>(1, 2048 / items));
    parts = std::max<int64_t>(1, std::min<int64_t>(parts, 65535));
    hipLaunchKernelGGL((msda_det_maxima_kernel<T, TL, A>), dim3((unsigned)items, (unsigned)parts), dim3(kDetThreads), 0, stream,
                       p, maxima);
    return check_launch("msda backward det maxima");
}

template <typename T, typename TL, typename A>
int det_scatter_any(const Params &p, const DetArgs &d, hipStream_t stream)
{
    const int64_t total = (int64_t)p.groups * p.Lq * p.M * ((int64_t)p.LA * p.PA + (int64_t)p.LB * p.PB) * p.D;
    hipLaunchKernelGGL((msda_det_scatter_kernel<T, TL, A>), dim3(det_blocks(total)), dim3(kDetThreads), 0, stream, p, d, total);
    return check_launch("msda backward det fixed-point scatter (any shape, int64 global atomics)");
}

template <typename T, typename A>
int det_convert(const Params &p, const DetArgs &d, hipStream_t stream)
{
    const int64_t elems = (int64_t)p.groups * p.S * p.M * p.D;
    if (p.gv_storage)
        hipLaunchKernelGGL((msda_det_convert_kernel<A, T>), dim3(det_blocks(elems)), dim3(kDetThreads), 0, stream,
                           p, d.maxima, d.acc, d.cls, static_cast<T *>(p.grad_value), elems);
    else
        hipLaunchKernelGGL((msda_det_convert_kernel<A, A>), dim3(det_blocks(elems)), dim3(kDetThreads), 0, stream,
                           p, d.maxima, d.acc, d.cls, static_cast<A *>(p.grad_value), elems);
    return check_launch("msda backward det convert");
}

}  // namespace

int launch_det_prepare(int dtype, const Params &p, void *workspace, DetArgs &d, hipStream_t stream)
{
    char *ws = static_cast<char *>(workspace);
    if (dtype == MSDA_F64) return det_prepare<double, double, double>(p, ws, d, stream);
    return dispatch_types(dtype, [&](auto t, auto tl) {
        return det_prepare<typename decltype(t)::type, typename decltype(tl)::type, float>(p, ws, d, stream);
    });
}

int launch_det_scatter_any(int dtype, const Params &p, const DetArgs &d, hipStream_t stream)
{
    if (dtype == MSDA_F64) return det_scatter_any<double, double, double>(p, d, stream);
    return dispatch_types(dtype, [&](auto t, auto tl) {
        return det_scatter_any<typename decltype(t)::type, typename decltype(tl)::type, float>(p, d, stream);
    });
}

int launch_det_convert(int dtype, const Params &p, const DetArgs &d, hipStream_t stream)
{
    if (dtype == MSDA_F64) return det_convert<double, double>(p, d, stream);
    return dispatch_types(dtype, [&](auto t, auto) { return det_convert<typename decltype(t)::type, float>(p, d, stream); });
}

}  // namespace msda
