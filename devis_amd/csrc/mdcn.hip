// mdcn.hip -- modulated deformable 2-D convolution (include/mdcn.h): the deformable im2col kernel, the backward kernel
// (grad_offset / grad_mask by a wavefront reduction over a group's channels, grad_input by float atomics into a
// channels-last accumulator) and their extern "C" entry points.  The products with the weights are the caller's GEMMs.
// gfx950, wave64, plain HIP.  The order-independent grad_input (mdcn_backward_input_fixed) is mdcn_det.hip; both units take
// a tap's corners and weights from mdcn_common.h.
#include "mdcn_common.h"

namespace mdcn {

thread_local Status err;

// V channels of one pixel as one naturally aligned load / store (16 bytes at V = 16 / sizeof(T))
template <typename T, int V> struct alignas(sizeof(T) * V) Pack { T v[V]; };


// ---- forward: deformable im2col ------------------------------------------------------------------------------
// One thread per (pixel, tap, V channels), channels fastest: a wave reads contiguous channel segments of the four
// corner rows and writes a contiguous run of the column buffer.
template <typename T, typename TO, int V>
__global__ __launch_bounds__(kThreads) void mdcn_im2col_kernel(const T *__restrict__ x, const TO *__restrict__ off,
                                                               const TO *__restrict__ msk, T *__restrict__ col,
                                                               const mdcn_shape s, const long long total)
{
    typedef typename Acc<T>::type A;
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= total) return;
    const int CV = s.C / V, K = s.Kh * s.Kw;
    const int c = (int)(t % CV) * V;
    const long long item = t / CV;          // (pixel, tap)
    const int k = (int)(item % K);
    const Tap<A> tap = locate<A, TO>(s, off, msk, item / K, k, c / (s.C / s.G));
    A acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = (A)0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (!tap.ok[q]) continue;
        const Pack<T, V> p = *reinterpret_cast<const Pack<T, V> *>(x + tap.row[q] + c);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] += tap.w[q] * (A)to_acc(p.v[e]);
    }
    Pack<T, V> o;
#pragma unroll
    for (int e = 0; e < V; ++e) from_acc(o.v[e], tap.m * acc[e]);
    *reinterpret_cast<Pack<T, V> *>(col + item * s.C + c) = o;
}

// ---- backward ------------------------------------------------------------------------------------------------
// One team of `team` lanes (a power of two <= 64, uniform over the launch) per (pixel, tap, group); lane l of a team
// takes the group's channels l, l + team, ...  So every atomic wave-instruction adds `team` CONTIGUOUS floats of one
// accumulator row per team (256 B at team = 64, two 128-B segments at 32), the shape that runs at the full atomic rate,
// and the three per-item sums (d/dy, d/dx, d/dmask) are a butterfly over the team's lanes: the same order every run.
template <typename T, typename TO>
__global__ __launch_bounds__(kThreads) void mdcn_backward_kernel(const T *__restrict__ x, const TO *__restrict__ off,
                                                                 const TO *__restrict__ msk, const T *__restrict__ gcol,
                                                                 typename Acc<T>::type *__restrict__ gin,
                                                                 TO *__restrict__ goff, TO *__restrict__ gmsk,
                                                                 const mdcn_shape s, const long long items,
                                                                 const int team, const int grads)
{
    typedef typename Acc<T>::type A;
    const int K = s.Kh * s.Kw, Cg = s.C / s.G;
    const int lane = threadIdx.x % team;
    long long item = (long long)blockIdx.x * (kThreads / team) + threadIdx.x / team;
    const bool live = item < items;         // a team past the end computes the last item and writes nothing
    if (!live) item = items - 1;
    const int g = (int)(item % s.G);
    const int k = (int)((item / s.G) % K);
    const long long pix = item / ((long long)s.G * K);
    const Tap<A> tap = locate<A, TO>(s, off, msk, pix, k, g);
    const bool want_in = (grads & MDCN_GRAD_INPUT) && live && tap.inside;
    const bool want_s = (grads & MDCN_GRAD_SAMPLING) && tap.inside;
    const T *gc_row = gcol + (pix * K + k) * s.C + g * Cg;
    const int c0 = g * Cg;
    A sy = (A)0, sx = (A)0, sm = (A)0;
    const A hy = (A)1 - tap.ly, hx = (A)1 - tap.lx;
    for (int c = lane; c < Cg; c += team) {
        const A gc = (A)to_acc(gc_row[c]);
        if (want_s) {
            A v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = tap.ok[q] ? (A)to_acc(x[tap.row[q] + c0 + c]) : (A)0;
            sm += gc * (tap.w[0] * v[0] + tap.w[1] * v[1] + tap.w[2] * v[2] + tap.w[3] * v[3]);
            sy += gc * (hx * (v[2] - v[0]) + tap.lx * (v[3] - v[1]));
            sx += gc * (hy * (v[1] - v[0]) + tap.ly * (v[3] - v[2]));
        }
        if (want_in) {
            const A gm = gc * tap.m;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (tap.ok[q]) atomicAdd(gin + tap.row[q] + c0 + c, gm * tap.w[q]);
        }
    }
    if (!(grads & MDCN_GRAD_SAMPLING)) return;      // (uniform over the launch)
    for (int d = team >> 1; d > 0; d >>= 1) {
        sy += __shfl_xor(sy, d, 64);
        sx += __shfl_xor(sx, d, 64);
        sm += __shfl_xor(sm, d, 64);
    }
    if (live && lane == 0) {
        const long long plane = (long long)s.Ho * s.Wo;
        from_acc(goff[tap.off_at], tap.m * sy);
        from_acc(goff[tap.off_at + plane], tap.m * sx);
        if (gmsk) from_acc(gmsk[tap.msk_at], sm);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------
int check_shape(const mdcn_shape *s)
{
    if (!s) return err.fail("null pointer: shape");
    if (s->N < 0 || s->C <= 0 || s->H <= 0 || s->W <= 0 || s->Ho <= 0 || s->Wo <= 0 || s->Kh <= 0 || s->Kw <= 0 ||
        s->stride_h <= 0 || s->stride_w <= 0 || s->dil_h <= 0 || s->dil_w <= 0 || s->G <= 0)
        return err.fail("sizes must be positive (N may be 0), padding not negative");
    if (s->pad_h < 0 || s->pad_w < 0) return err.fail("sizes must be positive (N may be 0), padding not negative");
    if (s->C % s->G) return err.fail("C = %lld is not a multiple of the offset groups G = %lld", s->C, s->G);
    const long long eh = (long long)s->H + 2LL * s->pad_h - (long long)s->dil_h * (s->Kh - 1) - 1;
    const long long ew = (long long)s->W + 2LL * s->pad_w - (long long)s->dil_w * (s->Kw - 1) - 1;
    if (eh < 0 || ew < 0 || eh / s->stride_h + 1 != s->Ho || ew / s->stride_w + 1 != s->Wo)
        return err.fail("Ho x Wo = %lld x %lld is not the output size of this convolution", s->Ho, s->Wo);
    return MDCN_OK;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the widest power of two <= limit that keeps a vector inside one offset group and 16-byte aligned
template <typename T> int vector_width(const mdcn_shape &s, const void *x, const void *col)
{
    const int full = 16 / (int)sizeof(T);
    return ((s.C / s.G) % full == 0 && aligned16(x) && aligned16(col)) ? full : 1;
}

template <typename T, typename TO>
int launch_im2col(const void *x, const void *off, const void *msk, const mdcn_shape &s, void *col, hipStream_t st)
{
    constexpr int full = 16 / (int)sizeof(T);
    const int V = vector_width<T>(s, x, col);
    const long long total = (long long)s.N * s.Ho * s.Wo * s.Kh * s.Kw * (s.C / V);
    unsigned blocks;
    if (err.grid_of(cdiv(total, kThreads), &blocks, kFewerImages)) return MDCN_ERR_ARGUMENT;
    if (V == full)
        hipLaunchKernelGGL((mdcn_im2col_kernel<T, TO, full>), dim3(blocks), dim3(kThreads), 0, st,
                           (const T *)x, (const TO *)off, (const TO *)msk, (T *)col, s, total);
    else
        hipLaunchKernelGGL((mdcn_im2col_kernel<T, TO, 1>), dim3(blocks), dim3(kThreads), 0, st,
                           (const T *)x, (const TO *)off, (const TO *)msk, (T *)col, s, total);
    return err.check_launch("mdcn_im2col_kernel");
}

// Lanes per (pixel, tap, group): among 32 and 64 the one that pads the group's channels least (ties: the wider, one
// 256-B segment per atomic instruction); a group of fewer than 32 channels gets the next power of two.
int team_size(int Cg)
{
    if (Cg <= 32) {
        int t = 1;
        while (t < Cg) t <<= 1;
        return t;
    }
    const int pad32 = (Cg + 31) / 32 * 32, pad64 = (Cg + 63) / 64 * 64;
    return pad64 <= pad32 ? 64 : 32;
}

template <typename T, typename TO>
int launch_backward(int grads, const void *x, const void *off, const void *msk, const void *gcol, const mdcn_shape &s,
                    void *gin, void *goff, void *gmsk, hipStream_t st)
{
    typedef typename Acc<T>::type A;
    const int team = team_size(s.C / s.G);
    const long long items = (long long)s.N * s.Ho * s.Wo * s.Kh * s.Kw * s.G;
    unsigned blocks;
    if (err.grid_of(cdiv(items, kThreads / team), &blocks, kFewerImages)) return MDCN_ERR_ARGUMENT;
    hipLaunchKernelGGL((mdcn_backward_kernel<T, TO>), dim3(blocks), dim3(kThreads), 0, st, (const T *)x,
                       (const TO *)off, (const TO *)msk, (const T *)gcol, (A *)gin, (TO *)goff, (TO *)gmsk, s, items, team,
                       grads);
    return err.check_launch("mdcn_backward_kernel");
}

}  // namespace mdcn

using namespace mdcn;

extern "C" {

int mdcn_version(void) { return MDCN_ABI_VERSION; }

const char *mdcn_last_error(void) { return err.msg; }

long long mdcn_workspace_bytes(int dtype, const mdcn_shape *shape, int batch)
{
    err.clear();
    if (check_dtype(dtype) != MDCN_OK) return MDCN_ERR_ARGUMENT;
    if (!shape) return err.fail("null pointer: shape");
    mdcn_shape s = *shape;
    s.N = 0;
    if (check_shape(&s) != MDCN_OK) return MDCN_ERR_ARGUMENT;
    if (batch < 0) return err.fail("sizes must be positive (N may be 0), padding not negative");
    return (long long)batch * s.Ho * s.Wo * s.Kh * s.Kw * s.C * elem_size(input_code(dtype));
}

int mdcn_im2col(int dtype, const void *input, const void *offset, const void *mask, const mdcn_shape *shape,
                void *columns, void *stream)
{
    err.clear();
    if (check_dtype(dtype) != MDCN_OK) return MDCN_ERR_ARGUMENT;
    if (check_shape(shape) != MDCN_OK) return MDCN_ERR_ARGUMENT;
    if (!input || !offset || !columns) return err.fail("null pointer: input, offset and columns are required");
    if (shape->N == 0) return MDCN_OK;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_types(dtype, [&](auto t, auto to) {
        return launch_im2col<type_of<decltype(t)>, type_of<decltype(to)>>(input, offset, mask, *shape, columns, st);
    });
}

int mdcn_backward(int grads, int dtype, const void *input, const void *offset, const void *mask,
                  const void *grad_columns, const mdcn_shape *shape, void *grad_input_acc, void *grad_offset,
                  void *grad_mask, void *stream)
{
    err.clear();
    if (check_dtype(dtype) != MDCN_OK) return MDCN_ERR_ARGUMENT;
    if (grads < 0 || grads > (MDCN_GRAD_INPUT | MDCN_GRAD_SAMPLING))
        return err.fail("grads = %lld is not a mask of MDCN_GRAD_INPUT and MDCN_GRAD_SAMPLING", grads);
    if (check_shape(shape) != MDCN_OK) return MDCN_ERR_ARGUMENT;
    if (!input || !offset || !grad_columns) return err.fail("null pointer: input, offset and grad_columns are required");
    if ((grads & MDCN_GRAD_INPUT) && !grad_input_acc) return err.fail("null pointer: grad_input_acc with MDCN_GRAD_INPUT");
    if ((grads & MDCN_GRAD_SAMPLING) && (!grad_offset || !grad_mask != !mask))
        return err.fail("null pointer: MDCN_GRAD_SAMPLING needs grad_offset, and grad_mask exactly when there is a mask");
    if (shape->N == 0 || grads == 0) return MDCN_OK;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_types(dtype, [&](auto t, auto to) {
        return launch_backward<type_of<decltype(t)>, type_of<decltype(to)>>(
            grads, input, offset, mask, grad_columns, *shape, grad_input_acc, grad_offset, grad_mask, st);
    });
}

}  // extern "C"
