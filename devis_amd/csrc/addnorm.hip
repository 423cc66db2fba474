// addnorm.hip -- the glue between the transformer layers' GEMMs (include/addnorm.h): LayerNorm(x +
// dropout(delta)) and dropout(relu(x)), forward and backward, each one pass.  gfx950, wave64, plain HIP.  One wave owns a row
// and holds it in registers; there is no LDS, no atomic and nothing is zeroed.  The dropout mask is Philox4x32-10 of (seed, row,
// channel / 4), recomputed by the backward, and the seed is read on the device.
#include "op_common.h"       // (fp contraction off)
#include "philox.h"
#include "addnorm.h"

namespace addnorm {

using namespace devis;

static_assert(ADDNORM_OK == kOk && ADDNORM_ERR_ARGUMENT == kErrArgument && ADDNORM_ERR_HIP == kErrHip, "status codes");
static_assert(ADDNORM_F32 == kF32 && ADDNORM_F64 == kF64 && ADDNORM_BF16 == kBF16 && ADDNORM_F16 == kF16, "dtype codes");

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxC = ADDNORM_MAX_CHANNELS;
constexpr int kChunkRows = 32;              // rows of one chunk of the backward's column sums
constexpr int kSpan = 256;                  // channels one group of four per lane covers: a row is G = ceil(C / kSpan) groups

thread_local Status err;     // addnorm_last_error()

// ---- the mask (include/addnorm.h; the generator is philox.h) ---------------------------------------------------------------
// bit j: element (row, 4 * quad + j) is kept
__device__ __forceinline__ unsigned keep_of(long long seed, long long row, unsigned quad, unsigned long long threshold)
{
    unsigned w[4];
    philox4x32_10((unsigned)seed, (unsigned)((unsigned long long)seed >> 32), (unsigned)row,
                  (unsigned)((unsigned long long)row >> 32), quad, 0u, w);
    unsigned keep = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) keep |= (unsigned long long)w[j] >= threshold ? 1u << j : 0u;
    return keep;
}

// ---- four consecutive elements --------------------------------------------------------------------------------------------
template <typename T> struct alignas(sizeof(T) * 4 > 16 ? 16 : sizeof(T) * 4) Quad {
    T v[4];
};

// p[0..3] -> out, elements at or beyond `n` as 0; one 8 / 16-byte access (two for double) when `vec`
template <typename T, typename A> __device__ __forceinline__ void load4(const T *p, int n, bool vec, A (&out)[4])
{
    if (vec) {
        if (n > 0) {
            const Quad<T> q = *reinterpret_cast<const Quad<T> *>(p);
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = (A)to_acc(q.v[j]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = (A)0;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = j < n ? (A)to_acc(p[j]) : (A)0;
    }
}

template <typename T, typename A> __device__ __forceinline__ void store4(T *p, int n, bool vec, const A (&in)[4])
{
    if (vec) {
        if (n > 0) {
            Quad<T> q;
#pragma unroll
            for (int j = 0; j < 4; ++j) from_acc(q.v[j], in[j]);
            *reinterpret_cast<Quad<T> *>(p) = q;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) from_acc(p[j], in[j]);
    }
}

// the first channel of group g of this lane
__device__ __forceinline__ int channel_of(int g, int lane) { return (g * 64 + lane) * 4; }

// ---- a row ------------------------------------------------------------------------------------------------------------------
// z = x + dropout(delta) of one row, channels >= C as 0; keep: bit g * 4 + j
template <typename TX, typename TD, int G, typename A>
__device__ __forceinline__ void row_of(const TX *__restrict__ x, const TD *__restrict__ delta, const long long *__restrict__ seed,
                                       long long row, int C, int lane, bool vec, unsigned long long threshold, A scale,
                                       A (&z)[G][4], unsigned &keep)
{
    keep = 0xffffffffu;
    if (seed) {
        const long long s = *seed;
        keep = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int c0 = channel_of(g, lane);
            if (c0 < C) keep |= keep_of(s, row, (unsigned)c0 >> 2, threshold) << (g * 4);
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c0 = channel_of(g, lane);
        A xa[4], da[4];
        load4(x + c0, C - c0, vec, xa);
        load4(delta + c0, C - c0, vec, da);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const A d = (keep >> (g * 4 + j)) & 1u ? da[j] * scale : (A)0;
            z[g][j] = xa[j] + d;
        }
    }
}

// the sum over the row's channels < C of v, in every lane: g, then j, ascending, then butterflies
template <int G, typename A> __device__ __forceinline__ A row_sum(const A (&v)[G][4], int C, int lane)
{
    A s = (A)0;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) s += channel_of(g, lane) + j < C ? v[g][j] : (A)0;
    return wave_sum(s);
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
template <typename TX, typename TD, typename TY, typename TP, int G>
__global__ __launch_bounds__(kThreads) void forward_kernel(const TX *__restrict__ x, const TD *__restrict__ delta,
                                                           const TP *__restrict__ weight, const TP *__restrict__ bias,
                                                           const long long *__restrict__ seed, TY *__restrict__ y,
                                                           typename Acc<TX>::type *__restrict__ mean_out,
                                                           typename Acc<TX>::type *__restrict__ rstd_out, const long long R,
                                                           const int C, const unsigned long long threshold,
                                                           const typename Acc<TX>::type scale, const typename Acc<TX>::type eps,
                                                           const int vec)
{
    typedef typename Acc<TX>::type A;
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (row >= R) return;
    A z[G][4];
    unsigned keep;
    row_of<TX, TD, G, A>(x + row * C, delta + row * C, seed, row, C, lane, vec != 0, threshold, scale, z, keep);
    const A mean = row_sum<G, A>(z, C, lane) / (A)C;
    A sq[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const A t = z[g][j] - mean;
            sq[g][j] = t * t;
        }
    const A var = row_sum<G, A>(sq, C, lane) / (A)C;
    const A rstd = rsqrt_of(var + eps);
    if (mean_out && lane == 0) {
        mean_out[row] = mean;
        rstd_out[row] = rstd;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c0 = channel_of(g, lane);
        A w[4], b[4], out[4];
        load4(weight + c0, C - c0, vec != 0, w);
        load4(bias + c0, C - c0, vec != 0, b);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = ((z[g][j] - mean) * rstd) * w[j] + b[j];
        store4(y + row * C + c0, C - c0, vec != 0, out);
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// Wave `chunk` owns the rows [chunk * kChunkRows, ...): grad_x and grad_delta of each, and the column partials of g * xhat and
// g, rows ascending, -> ws[(chunk * 2 + which) * C + c], or the results themselves when the call is one chunk.
template <typename TX, typename TD, typename TY, typename TP, int G>
__global__ __launch_bounds__(kThreads) void backward_kernel(const TX *__restrict__ x, const TD *__restrict__ delta,
                                                            const TP *__restrict__ weight, const long long *__restrict__ seed,
                                                            const typename Acc<TX>::type *__restrict__ mean,
                                                            const typename Acc<TX>::type *__restrict__ rstd,
                                                            const TY *__restrict__ grad_y, TX *__restrict__ grad_x,
                                                            TD *__restrict__ grad_delta, typename Acc<TX>::type *__restrict__ ws,
                                                            TP *__restrict__ grad_weight, TP *__restrict__ grad_bias,
                                                            const long long R, const int C, const int chunks,
                                                            const unsigned long long threshold,
                                                            const typename Acc<TX>::type scale, const int vec)
{
    typedef typename Acc<TX>::type A;
    const int lane = threadIdx.x & 63;
    const long long chunk = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (chunk >= chunks) return;
    const bool want_dz = grad_x || grad_delta, want_params = grad_weight || grad_bias;
    const long long row0 = chunk * kChunkRows;
    const long long row1 = R - row0 < kChunkRows ? R : row0 + kChunkRows;
    A w[G][4], pw[G][4], pb[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c0 = channel_of(g, lane);
        load4(weight + c0, want_dz ? C - c0 : 0, vec != 0, w[g]);
#pragma unroll
        for (int j = 0; j < 4; ++j) pw[g][j] = pb[g][j] = (A)0;
    }
    for (long long row = row0; row < row1; ++row) {
        A z[G][4], gy[G][4];
        unsigned keep;
        row_of<TX, TD, G, A>(x + row * C, delta + row * C, seed, row, C, lane, vec != 0, threshold, scale, z, keep);
        const A m = mean[row], rs = rstd[row];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int c0 = channel_of(g, lane);
            load4(grad_y + row * C + c0, C - c0, vec != 0, gy[g]);
#pragma unroll
            for (int j = 0; j < 4; ++j) z[g][j] = (z[g][j] - m) * rs;          // xhat, the forward's bits
        }
        if (want_params) {
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    pw[g][j] += gy[g][j] * z[g][j];
                    pb[g][j] += gy[g][j];
                }
        }
        if (want_dz) {
            A gw[G][4], gwx[G][4];
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    gw[g][j] = gy[g][j] * w[g][j];
                    gwx[g][j] = gw[g][j] * z[g][j];
                }
            const A c1 = row_sum<G, A>(gw, C, lane) / (A)C;
            const A c2 = row_sum<G, A>(gwx, C, lane) / (A)C;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int c0 = channel_of(g, lane);
                A dz[4], dd[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    dz[j] = ((gw[g][j] - c1) - z[g][j] * c2) * rs;
                    dd[j] = (keep >> (g * 4 + j)) & 1u ? dz[j] * scale : (A)0;
                }
                if (grad_x) store4(grad_x + row * C + c0, C - c0, vec != 0, dz);
                if (grad_delta) store4(grad_delta + row * C + c0, C - c0, vec != 0, dd);
            }
        }
    }
    if (!want_params) return;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c0 = channel_of(g, lane);
        if (chunks == 1) {
            if (grad_weight) store4(grad_weight + c0, C - c0, vec != 0, pw[g]);
            if (grad_bias) store4(grad_bias + c0, C - c0, vec != 0, pb[g]);
        } else {                                            // (the workspace is 16-byte aligned and C % 4 == 0 when vec)
            store4(ws + (chunk * 2 + 0) * C + c0, C - c0, vec != 0, pw[g]);
            store4(ws + (chunk * 2 + 1) * C + c0, C - c0, vec != 0, pb[g]);
        }
    }
}

// One thread per column and sum: the chunks ascending, rounded once.
template <typename A, typename TP>
__global__ __launch_bounds__(64) void combine_kernel(const A *__restrict__ ws, TP *__restrict__ grad_weight,
                                                     TP *__restrict__ grad_bias, const int C, const int chunks)
{
    const int c = blockIdx.x * 64 + threadIdx.x, which = blockIdx.y;
    TP *dst = which ? grad_bias : grad_weight;
    if (c >= C || !dst) return;
    const A *src = ws + (long long)which * C + c;
    A s = src[0];
#pragma unroll 8
    for (int k = 1; k < chunks; ++k) s += src[(long long)k * 2 * C];
    from_acc(dst[c], s);
}

// ---- the relu pass ----------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void relu_forward_kernel(const T *__restrict__ x, const long long *__restrict__ seed,
                                                                T *__restrict__ y, const long long quads, const int C,
                                                                const int quads_per_row, const unsigned long long threshold,
                                                                const typename Acc<T>::type scale, const int vec)
{
    typedef typename Acc<T>::type A;
    const long long q = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (q >= quads) return;
    const long long row = q / quads_per_row;
    const int quad = (int)(q - row * quads_per_row), c0 = quad * 4;
    const unsigned keep = seed ? keep_of(*seed, row, (unsigned)quad, threshold) : 0xfu;
    A v[4], out[4];
    load4(x + row * C + c0, C - c0, vec != 0, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const A kept = v[j] > (A)0 ? v[j] * scale : (v[j] != v[j] ? v[j] : (A)0);
        out[j] = (keep >> j) & 1u ? kept : (A)0;
    }
    store4(y + row * C + c0, C - c0, vec != 0, out);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void relu_backward_kernel(const T *__restrict__ y, const T *__restrict__ grad_y,
                                                                 T *__restrict__ grad_x, const long long n,
                                                                 const typename Acc<T>::type scale, const int vec)
{
    typedef typename Acc<T>::type A;
    const long long e = ((long long)blockIdx.x * kThreads + threadIdx.x) * 4;
    if (e >= n) return;
    const int left = n - e < 4 ? (int)(n - e) : 4;
    A v[4], g[4], out[4];
    load4(y + e, left, vec != 0, v);
    load4(grad_y + e, left, vec != 0, g);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = v[j] > (A)0 ? g[j] * scale : (A)0;
    store4(grad_x + e, left, vec != 0, out);
}

// ---- host -------------------------------------------------------------------------------------------------------------------
int check_shape(const addnorm_shape *s, bool norm)
{
    if (!s) return err.fail("null pointer: shape");
    if (s->R < 0) return err.fail("R must not be negative");
    if (s->R > 0x7fffffffLL) return err.fail("R = %lld does not fit 31 bits", s->R);
    if (s->C < 1) return err.fail("C must be positive, got %lld", s->C);
    if (norm && s->C > kMaxC) return err.fail("C = %lld is more than the %lld channels a wave holds", s->C, kMaxC);
    return ADDNORM_OK;
}

// p -> threshold and scale (include/addnorm.h)
int mask_of(double p, const long long *seed, unsigned long long *threshold, double *scale)
{
    if (!(p >= 0.0 && p <= 1.0)) return err.fail("p must be in [0, 1]");
    if (p > 0.0 && !seed) return err.fail("null pointer: seed is required when p > 0");
    *threshold = (unsigned long long)(p * 4294967296.0);        // (the product is exact or rounds down to below 2^32 + 1)
    *scale = p < 1.0 ? 1.0 / (1.0 - p) : 0.0;
    return ADDNORM_OK;
}

bool is16(int d) { return d == kBF16 || d == kF16; }

int check_types(const addnorm_types *t)
{
    if (!t) return err.fail("null pointer: types");
    if (!elem_size(t->x) || !elem_size(t->delta) || !elem_size(t->y) || !elem_size(t->param)) return err.fail("bad dtype code");
    const bool same = t->x == t->delta && t->x == t->y;
    const bool ok = (same && (t->param == t->x || (is16(t->x) && t->param == kF32))) ||
                    (t->x == kF32 && is16(t->delta) && t->y == kF32 && t->param == kF32) ||
                    (is16(t->x) && t->delta == t->x && t->y == kF32 && (t->param == t->x || t->param == kF32));
    return ok ? ADDNORM_OK : err.fail("unsupported combination of dtypes (x %lld, delta %lld; see addnorm.h)", t->x, t->delta);
}

// f(Tag<TX>, Tag<TD>, Tag<TY>, Tag<TP>) of a checked combination
template <typename H, typename F> int dispatch16(const addnorm_types &t, F &&f)
{
    const bool wide_y = t.y == kF32, wide_p = t.param == kF32;
    if (wide_y) return wide_p ? f(Tag<H>(), Tag<H>(), Tag<float>(), Tag<float>()) : f(Tag<H>(), Tag<H>(), Tag<float>(), Tag<H>());
    return wide_p ? f(Tag<H>(), Tag<H>(), Tag<H>(), Tag<float>()) : f(Tag<H>(), Tag<H>(), Tag<H>(), Tag<H>());
}

template <typename F> int dispatch_types(const addnorm_types &t, F &&f)
{
    if (t.x == kF64) return f(Tag<double>(), Tag<double>(), Tag<double>(), Tag<double>());
    if (t.x == kF32) {
        if (t.delta == kF32) return f(Tag<float>(), Tag<float>(), Tag<float>(), Tag<float>());
        return t.delta == kBF16 ? f(Tag<float>(), Tag<__hip_bfloat16>(), Tag<float>(), Tag<float>())
                                : f(Tag<float>(), Tag<__half>(), Tag<float>(), Tag<float>());
    }
    return t.x == kBF16 ? dispatch16<__hip_bfloat16>(t, f) : dispatch16<__half>(t, f);
}

template <int N> struct Groups { static constexpr int value = N; };

// f(Groups<G>) for the G in {1, 2, 4} that covers C channels
template <typename F> int dispatch_groups(int C, F &&f)
{
    if (C <= kSpan) return f(Groups<1>());
    return C <= 2 * kSpan ? f(Groups<2>()) : f(Groups<4>());
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }       // (NULL is aligned)

int chunks_of(const addnorm_shape &s) { return (int)cdiv(s.R, kChunkRows); }

}  // namespace addnorm

using namespace addnorm;

extern "C" {

int addnorm_version(void) { return ADDNORM_ABI_VERSION; }

const char *addnorm_last_error(void) { return err.msg; }

int addnorm_tile(int which)
{
    switch (which) {
    case ADDNORM_TILE_ROWS: return kChunkRows;
    case ADDNORM_TILE_CHANNELS: return kMaxC;
    default: return -1;
    }
}

long long addnorm_workspace_bytes(int x_dtype, const addnorm_shape *shape)
{
    err.clear();
    if (!elem_size(x_dtype)) return err.fail("bad dtype code %lld", x_dtype);
    if (check_shape(shape, true) != ADDNORM_OK) return ADDNORM_ERR_ARGUMENT;
    const int chunks = chunks_of(*shape);
    const long long bytes = chunks > 1 ? (long long)chunks * 2 * shape->C * acc_size(x_dtype) : 0;
    return (bytes + 255) / 256 * 256;
}

int addnorm_forward(const addnorm_types *types, const void *x, const void *delta, const void *weight, const void *bias,
                    const long long *seed, double p, double eps, const addnorm_shape *shape, void *y, void *mean, void *rstd,
                    void *stream)
{
    err.clear();
    if (check_types(types) != ADDNORM_OK || check_shape(shape, true) != ADDNORM_OK) return ADDNORM_ERR_ARGUMENT;
    unsigned long long threshold;
    double scale;
    if (mask_of(p, seed, &threshold, &scale) != ADDNORM_OK) return ADDNORM_ERR_ARGUMENT;
    if (!(eps == eps)) return err.fail("eps must be a number");
    const addnorm_shape &s = *shape;
    if (s.R == 0) return ADDNORM_OK;
    if (!x || !delta || !weight || !bias || !y) return err.fail("null pointer: x, delta, weight, bias and y are required");
    if (!mean != !rstd) return err.fail("null pointer: mean and rstd are given together or not at all");
    const int vec = s.C % 4 == 0 && aligned16(x) && aligned16(delta) && aligned16(weight) && aligned16(bias) && aligned16(y);
    unsigned grid;
    if (err.grid_of(cdiv(s.R, kWaves), &grid) != ADDNORM_OK) return ADDNORM_ERR_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    const long long *sd = p > 0.0 ? seed : nullptr;
    return dispatch_types(*types, [&](auto tx, auto td, auto ty, auto tp) {
        typedef type_of<decltype(tx)> TX;
        typedef type_of<decltype(td)> TD;
        typedef type_of<decltype(ty)> TY;
        typedef type_of<decltype(tp)> TP;
        typedef typename Acc<TX>::type A;
        return dispatch_groups(s.C, [&](auto groups) {
            constexpr int G = decltype(groups)::value;
            hipLaunchKernelGGL((forward_kernel<TX, TD, TY, TP, G>), dim3(grid), dim3(kThreads), 0, st, (const TX *)x,
                               (const TD *)delta, (const TP *)weight, (const TP *)bias, sd, (TY *)y, (A *)mean, (A *)rstd, s.R,
                               s.C, threshold, (A)scale, (A)eps, vec);
            return err.check_launch("addnorm_forward");
        });
    });
}

int addnorm_backward(const addnorm_types *types, const void *x, const void *delta, const void *weight, const long long *seed,
                     double p, const void *mean, const void *rstd, const void *grad_y, const addnorm_shape *shape,
                     void *workspace, void *grad_x, void *grad_delta, void *grad_weight, void *grad_bias, void *stream)
{
    err.clear();
    if (check_types(types) != ADDNORM_OK || check_shape(shape, true) != ADDNORM_OK) return ADDNORM_ERR_ARGUMENT;
    unsigned long long threshold;
    double scale;
    if (mask_of(p, seed, &threshold, &scale) != ADDNORM_OK) return ADDNORM_ERR_ARGUMENT;
    if (!grad_x && !grad_delta && !grad_weight && !grad_bias) return err.fail("no gradient is asked for");
    const addnorm_shape &s = *shape;
    if (s.R == 0) return ADDNORM_OK;
    if (!x || !delta || !mean || !rstd || !grad_y) return err.fail("null pointer: x, delta, mean, rstd and grad_y are required");
    if ((grad_x || grad_delta) && !weight) return err.fail("null pointer: weight is required for grad_x and grad_delta");
    const int chunks = chunks_of(s);
    const bool params = grad_weight || grad_bias;
    if (params && chunks > 1 && !workspace) return err.fail("null pointer: workspace is required when the column sums span chunks");
    if (!aligned16(workspace)) return err.fail("the workspace must be 16-byte aligned");
    const int vec = s.C % 4 == 0 && aligned16(x) && aligned16(delta) && aligned16(weight) && aligned16(grad_y) &&
                    aligned16(grad_x) && aligned16(grad_delta) && aligned16(grad_weight) && aligned16(grad_bias);
    hipStream_t st = (hipStream_t)stream;
    const long long *sd = p > 0.0 ? seed : nullptr;
    return dispatch_types(*types, [&](auto tx, auto td, auto ty, auto tp) {
        typedef type_of<decltype(tx)> TX;
        typedef type_of<decltype(td)> TD;
        typedef type_of<decltype(ty)> TY;
        typedef type_of<decltype(tp)> TP;
        typedef typename Acc<TX>::type A;
        return dispatch_groups(s.C, [&](auto groups) {
            constexpr int G = decltype(groups)::value;
            hipLaunchKernelGGL((backward_kernel<TX, TD, TY, TP, G>), dim3((unsigned)cdiv(chunks, kWaves)), dim3(kThreads), 0, st,
                               (const TX *)x, (const TD *)delta, (const TP *)weight, sd, (const A *)mean, (const A *)rstd,
                               (const TY *)grad_y, (TX *)grad_x, (TD *)grad_delta, (A *)workspace, (TP *)grad_weight,
                               (TP *)grad_bias, s.R, s.C, chunks, threshold, (A)scale, vec);
            if (params && chunks > 1)
                hipLaunchKernelGGL((combine_kernel<A, TP>), dim3((unsigned)cdiv(s.C, 64), 2), dim3(64), 0, st,
                                   (const A *)workspace, (TP *)grad_weight, (TP *)grad_bias, s.C, chunks);
            return err.check_launch("addnorm_backward");
        });
    });
}

int addnorm_relu_forward(int dtype, const void *x, const long long *seed, double p, const addnorm_shape *shape, void *y,
                         void *stream)
{
    err.clear();
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (check_shape(shape, false) != ADDNORM_OK) return ADDNORM_ERR_ARGUMENT;
    unsigned long long threshold;
    double scale;
    if (mask_of(p, seed, &threshold, &scale) != ADDNORM_OK) return ADDNORM_ERR_ARGUMENT;
    const addnorm_shape &s = *shape;
    if (s.R == 0) return ADDNORM_OK;
    if (!x || !y) return err.fail("null pointer: x and y are required");
    const int quads_per_row = (int)cdiv(s.C, 4);
    const long long quads = s.R * quads_per_row;
    unsigned grid;
    if (err.grid_of(cdiv(quads, kThreads), &grid) != ADDNORM_OK) return ADDNORM_ERR_ARGUMENT;
    const int vec = s.C % 4 == 0 && aligned16(x) && aligned16(y);
    hipStream_t st = (hipStream_t)stream;
    const long long *sd = p > 0.0 ? seed : nullptr;
    const int C = s.C;
    return dispatch(dtype, [&](auto t) {
        typedef type_of<decltype(t)> T;
        typedef typename Acc<T>::type A;
        hipLaunchKernelGGL((relu_forward_kernel<T>), dim3(grid), dim3(kThreads), 0, st, (const T *)x, sd, (T *)y, quads, C,
                           quads_per_row, threshold, (A)scale, vec);
        return err.check_launch("addnorm_relu_forward");
    });
}

int addnorm_relu_backward(int dtype, const void *y, const void *grad_y, double p, long long n, void *grad_x, void *stream)
{
    err.clear();
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (n < 0) return err.fail("n must not be negative");
    if (!(p >= 0.0 && p <= 1.0)) return err.fail("p must be in [0, 1]");
    if (n == 0) return ADDNORM_OK;
    if (!y || !grad_y || !grad_x) return err.fail("null pointer: y, grad_y and grad_x are required");
    unsigned grid;
    if (err.grid_of(cdiv(cdiv(n, 4), kThreads), &grid) != ADDNORM_OK) return ADDNORM_ERR_ARGUMENT;
    const int vec = n % 4 == 0 && aligned16(y) && aligned16(grad_y) && aligned16(grad_x);
    const double scale = p < 1.0 ? 1.0 / (1.0 - p) : 0.0;
    hipStream_t st = (hipStream_t)stream;
    return dispatch(dtype, [&](auto t) {
        typedef type_of<decltype(t)> T;
        typedef typename Acc<T>::type A;
        hipLaunchKernelGGL((relu_backward_kernel<T>), dim3(grid), dim3(kThreads), 0, st, (const T *)y, (const T *)grad_y,
                           (T *)grad_x, n, (A)scale, vec);
        return err.check_launch("addnorm_relu_backward");
    });
}

}  // extern "C"
