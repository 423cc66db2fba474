// mdcn_det.hip -- grad_input of the modulated deformable convolution whose every element depends only on the multiset of
// terms that reach it (include/mdcn.h, mdcn_backward_input_fixed): the opt-in order-independent backward.
//
// Float sums depend on their order, integer sums do not.  Every term  (grad_columns * mask) * w_corner  -- the operand of
// mdcn_backward_kernel's atomicAdd, evaluated left to right with explicit round-to-nearest products -- is rounded to
// nearest-even onto a multiple of a quantum q = 2^e and added as int64; the element is acc * q, rounded once to the
// arithmetic type.  q is fixed per IMAGE from A = max |mask| (1 without a mask) and G = max |grad_columns| over the image's
// finite values and n = Ho*Wo*Kh*Kw, the terms an element can receive at most (a tap's four corners are four different
// pixels): the smallest power of two with A * G * n <= 2^62 * q (msda_det.h, det_exponent), so no sum overflows.  Everything
// q depends on is the image's own data: an image's gradient is the same alone or in a batch, under any chunking, launch
// geometry or team size.  Non-finite terms set bits of a per-element class nibble (NaN, +Inf, -Inf), combined by OR: the
// element is then what IEEE summation gives.
//
// Kernels, all on the stream of the call:
//   maxima    grid (image, part): max of the finite |mask| and |grad_columns| bits, one 64-bit atomic max per wave;
//   scatter   the team shape of mdcn_backward_kernel: one team per (pixel, tap, group), lane = channel, so a wave
//             instruction adds `team` contiguous int64 of one accumulator row (512 B at team = 64); zero addends are skipped;
//   convert   accumulators and nibbles -> [N, H, W, C] in the arithmetic type, every element written.
// Workspace (mdcn_fixed_workspace_bytes): [N*H*W*C] int64 accumulators, [ceil(N*H*W*C / 8)] u32 class words (4 bits per
// element), [N * 2] u64 maxima, each part 256-B aligned; zeroed on the stream first.
#include "mdcn_common.h"
#include "msda_det.h"

namespace mdcn {
namespace {

using msda::DetBits;

long long round256(long long bytes) { return (bytes + 255) / 256 * 256; }

struct FixedLayout {
    long long acc, cls, maxima, total;      // byte offsets of the three parts, and the size of all of them
};

FixedLayout fixed_layout(const mdcn_shape &s, long long batch)
{
    const long long elems = batch * s.H * s.W * s.C;
    FixedLayout l;
    l.acc = 0;
    l.cls = round256(elems * 8);
    l.maxima = l.cls + round256((elems + 7) / 8 * 4);
    l.total = l.maxima + round256(batch * 16);
    return l;
}

__device__ __forceinline__ long long terms_bound(const mdcn_shape &s)
{
    return (long long)s.Ho * s.Wo * s.Kh * s.Kw;
}

// grid (N, parts): workgroup `blockIdx.y` of image `blockIdx.x` strides over the image's mask and grad_columns rows.
// maxima[2n] = bits of the largest finite |mask| (of 1 without a mask), maxima[2n + 1] = of the largest finite |grad_columns|;
// unsigned order is magnitude order for non-negative floats, and a max does not depend on the order it is taken in.
template <typename T, typename TO>
__global__ __launch_bounds__(kThreads) void mdcn_fixed_maxima_kernel(const TO *__restrict__ msk, const T *__restrict__ gcol,
                                                                     unsigned long long *__restrict__ maxima,
                                                                     const mdcn_shape s)
{
    typedef typename Acc<T>::type A;
    const long long n = blockIdx.x;
    const long long stride = (long long)gridDim.y * kThreads, start = (long long)blockIdx.y * kThreads + threadIdx.x;
    const long long P = (long long)s.Ho * s.Wo, K = (long long)s.Kh * s.Kw;
    unsigned long long amax = msk ? 0ull : msda::det_abs_bits<A>((A)1), gmax = 0;
    if (msk) {
        const TO *m = msk + n * s.G * K * P;
        for (long long j = start; j < s.G * K * P; j += stride) {
            const unsigned long long v = msda::det_abs_bits<A>((A)to_acc(m[j]));
            amax = v > amax ? v : amax;
        }
    }
    const T *gc = gcol + n * P * K * s.C;
    for (long long j = start; j < P * K * s.C; j += stride) {
        const unsigned long long v = msda::det_abs_bits<A>((A)to_acc(gc[j]));
        gmax = v > gmax ? v : gmax;
    }
    amax = wave_max(amax);
    gmax = wave_max(gmax);
    if ((threadIdx.x & 63) == 0) {
        atomicMax(maxima + 2 * n, amax);
        atomicMax(maxima + 2 * n + 1, gmax);
    }
}

// One team of `team` lanes per (pixel, tap, group), lane l takes the group's channels l, l + team, ... as in
// mdcn_backward_kernel; the terms are that kernel's atomicAdd operands, formed from the same Tap.
template <typename T, typename TO>
__global__ __launch_bounds__(kThreads) void mdcn_fixed_scatter_kernel(const TO *__restrict__ off, const TO *__restrict__ msk,
                                                                      const T *__restrict__ gcol,
                                                                      const unsigned long long *__restrict__ maxima,
                                                                      long long *__restrict__ acc, unsigned *__restrict__ cls,
                                                                      const mdcn_shape s, const long long items, const int team)
{
    typedef typename Acc<T>::type A;
    const int K = s.Kh * s.Kw, Cg = s.C / s.G;
    const int lane = threadIdx.x % team;
    const long long item = (long long)blockIdx.x * (kThreads / team) + threadIdx.x / team;
    if (item >= items) return;
    const int g = (int)(item % s.G);
    const int k = (int)((item / s.G) % K);
    const long long pix = item / ((long long)s.G * K);
    const Tap<A> tap = locate<A, TO>(s, off, msk, pix, k, g);
    if (!tap.inside) return;
    const int e = msda::det_exponent<A>(maxima + 2 * (pix / ((long long)s.Ho * s.Wo)), terms_bound(s));
    const T *gc_row = gcol + (pix * K + k) * s.C + g * Cg;
    const int c0 = g * Cg;
    for (int c = lane; c < Cg; c += team) {
        const A gm = DetBits<A>::mul((A)to_acc(gc_row[c]), tap.m);      // (tap.m is 1 without a mask: the product is exact)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!tap.ok[q]) continue;
            const A term = DetBits<A>::mul(gm, tap.w[q]);
            const long long el = tap.row[q] + c0 + c;
            if (!msda::det_finite<A>(term)) {
                atomicOr(cls + (el >> 3), msda::det_class<A>(term) << ((el & 7) * 4));
            } else {
                const long long v = msda::det_fixed<A>(term, e);
                if (v) atomicAdd(reinterpret_cast<unsigned long long *>(acc + el), (unsigned long long)v);
            }
        }
    }
}

template <typename A>
__global__ __launch_bounds__(kThreads) void mdcn_fixed_convert_kernel(const unsigned long long *__restrict__ maxima,
                                                                      const long long *__restrict__ acc,
                                                                      const unsigned *__restrict__ cls, A *__restrict__ out,
                                                                      const mdcn_shape s, const long long total)
{
    const long long image = (long long)s.H * s.W * s.C;
    long long n_of_e = -1;      // the image `e` belongs to: a thread's elements mostly stay in one image
    int e = 0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
        const unsigned k = (cls[i >> 3] >> ((i & 7) * 4)) & 7u;
        A v;
        if ((k & 1) || (k & 6) == 6) {
            v = (A)NAN;
        } else if (k) {
            v = k == 2 ? (A)INFINITY : -(A)INFINITY;
        } else {
            const long long n = i / image;
            if (n != n_of_e) {
                e = msda::det_exponent<A>(maxima + 2 * n, terms_bound(s));
                n_of_e = n;
            }
            v = DetBits<A>::ldexp_((A)acc[i], e);       // one rounding (int64 -> A); the scaling is exact but at the range ends
        }
        out[i] = v;
    }
}

template <typename T, typename TO>
int launch_fixed(const void *off, const void *msk, const void *gcol, const mdcn_shape &s, void *workspace, void *gin,
                 hipStream_t st)
{
    typedef typename Acc<T>::type A;
    const FixedLayout l = fixed_layout(s, s.N);
    char *ws = static_cast<char *>(workspace);
    long long *acc = reinterpret_cast<long long *>(ws + l.acc);
    unsigned *cls = reinterpret_cast<unsigned *>(ws + l.cls);
    unsigned long long *maxima = reinterpret_cast<unsigned long long *>(ws + l.maxima);
    const int team = team_size(s.C / s.G);
    const long long items = (long long)s.N * s.Ho * s.Wo * s.Kh * s.Kw * s.G;
    unsigned blocks;
    if (err.grid_of(cdiv(items, kThreads / team), &blocks, kFewerImages)) return MDCN_ERR_ARGUMENT;
    const hipError_t zeroed = hipMemsetAsync(ws, 0, (size_t)l.total, st);
    if (zeroed != hipSuccess) return err.fail_hip("mdcn_backward_input_fixed: hipMemsetAsync(workspace)", zeroed);

    // (image, part) workgroups: parts so that a batch covers the chip about twice; an image's maxima do not depend on the split
    const long long per_image = (long long)s.Ho * s.Wo * s.Kh * s.Kw * s.C;
    long long parts = (per_image + 4 * kThreads - 1) / (4 * kThreads);
    const long long spread = 2048 / s.N > 1 ? 2048 / s.N : 1;
    parts = parts < spread ? parts : spread;
    parts = parts < 1 ? 1 : (parts > 65535 ? 65535 : parts);
    hipLaunchKernelGGL((mdcn_fixed_maxima_kernel<T, TO>), dim3((unsigned)s.N, (unsigned)parts), dim3(kThreads), 0, st,
                       (const TO *)msk, (const T *)gcol, maxima, s);
    int rc = err.check_launch("mdcn_fixed_maxima_kernel");
    if (rc != MDCN_OK) return rc;
    hipLaunchKernelGGL((mdcn_fixed_scatter_kernel<T, TO>), dim3(blocks), dim3(kThreads), 0, st, (const TO *)off,
                       (const TO *)msk, (const T *)gcol, maxima, acc, cls, s, items, team);
    rc = err.check_launch("mdcn_fixed_scatter_kernel");
    if (rc != MDCN_OK) return rc;
    const long long total = (long long)s.N * s.H * s.W * s.C;
    const long long want = (total + kThreads - 1) / kThreads;
    hipLaunchKernelGGL((mdcn_fixed_convert_kernel<A>), dim3((unsigned)(want < 65536 * 16 ? want : 65536 * 16)), dim3(kThreads),
                       0, st, maxima, acc, cls, (A *)gin, s, total);
    return err.check_launch("mdcn_fixed_convert_kernel");
}

}  // namespace
}  // namespace mdcn

using namespace mdcn;

extern "C" {

long long mdcn_fixed_workspace_bytes(int dtype, const mdcn_shape *shape, int batch)
{
    err.clear();
    if (check_dtype(dtype) != MDCN_OK) return MDCN_ERR_ARGUMENT;
    if (!shape) return err.fail("null pointer: shape");
    mdcn_shape s = *shape;
    s.N = 0;
    if (check_shape(&s) != MDCN_OK) return MDCN_ERR_ARGUMENT;
    if (batch < 0) return err.fail("sizes must be positive (N may be 0), padding not negative");
    return fixed_layout(s, batch).total;
}

int mdcn_backward_input_fixed(int dtype, const void *offset, const void *mask, const void *grad_columns,
                              const mdcn_shape *shape, void *workspace, void *grad_input, void *stream)
{
    err.clear();
    if (check_dtype(dtype) != MDCN_OK) return MDCN_ERR_ARGUMENT;
    if (check_shape(shape) != MDCN_OK) return MDCN_ERR_ARGUMENT;
    if (!offset || !grad_columns || !workspace || !grad_input)
        return err.fail("null pointer: offset, grad_columns, workspace and grad_input are required");
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return err.fail("workspace must be 256-byte aligned");
    if (shape->N == 0) return MDCN_OK;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_types(dtype, [&](auto t, auto to) {
        return launch_fixed<type_of<decltype(t)>, type_of<decltype(to)>>(offset, mask, grad_columns, *shape, workspace,
                                                                                     grad_input, st);
    });
}

}  // extern "C"
