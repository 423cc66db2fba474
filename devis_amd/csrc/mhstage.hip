// mhstage.hip -- one stage of the mask head's glue (include/mhstage.h): GroupNorm, ReLU, nearest
// upsampling, the FPN add and the concatenation of the attention maps in a statistics pass and an apply pass, and the
// stage's backward.  gfx950, wave64, plain HIP, fp32 arithmetic (fp64 for doubles); no atomics: every sum has a fixed order.
//
// The kernels are templates of the storage type of x alone.  Whether weight / bias, extra and out are float32 beside a
// 16-bit x is a kernel argument: a wave-uniform branch around a load or a store, not a compile-time variant.
#include "op_common.h"
#include "mhstage.h"

namespace mhstage {

using namespace devis;

static_assert(MHSTAGE_OK == kOk && MHSTAGE_ERR_ARGUMENT == kErrArgument && MHSTAGE_ERR_HIP == kErrHip, "status codes");
static_assert(MHSTAGE_F32 == kF32 && MHSTAGE_F64 == kF64 && MHSTAGE_BF16 == kBF16 && MHSTAGE_F16 == kF16, "dtype codes");

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kStatPer = 16;                    // elements per lane of a statistics tile, held in registers
constexpr int kStatTile = kThreads * kStatPer;
constexpr int kTP = 64;                         // apply: destination pixels per workgroup (one per lane)
constexpr int kTC = 32;                         // apply: channels per workgroup (kTC / kWaves per wave)
constexpr int kBP = 4;                          // backward pass 1: source pixels per lane
constexpr int kBwdPixels = 64 * kBP;
constexpr int kBC = 16;                         // backward pass 1: channels per workgroup
constexpr int kGxPer = 4;                       // backward pass 2: elements per lane

thread_local Status err;     // mhstage_last_error()

// PyTorch's mode="nearest" source index (include/mhstage.h), in float32 for every dtype
__device__ __forceinline__ int src_index(int d, int in, int out)
{
    const float scale = (float)in / (float)out;
    const int s = (int)floorf((float)d * scale);
    return s < in - 1 ? s : in - 1;
}

// the first d in [0, out] with src_index(d) >= s (out when there is none); src_index is monotone in d
__device__ __forceinline__ int first_dest(int s, int in, int out)
{
    int d = (int)((float)s * ((float)out / (float)in));
    d = d < 0 ? 0 : (d > out ? out : d);
    while (d > 0 && src_index(d - 1, in, out) >= s) --d;
    while (d < out && src_index(d, in, out) < s) ++d;
    return d;
}

// a tensor that is float32 (`wide`) or T
template <typename T> __device__ __forceinline__ typename Acc<T>::type ld(const void *p, long long i, bool wide)
{
    typedef typename Acc<T>::type A;
    return wide ? (A) reinterpret_cast<const float *>(p)[i] : (A)to_acc(reinterpret_cast<const T *>(p)[i]);
}
template <typename T> __device__ __forceinline__ void st(void *p, long long i, typename Acc<T>::type v, bool wide)
{
    if (wide) reinterpret_cast<float *>(p)[i] = (float)v;
    else from_acc(reinterpret_cast<T *>(p)[i], v);
}

__device__ __forceinline__ long long index_at(const void *idx, int is64, long long n)
{
    if (!idx) return n;
    return is64 ? reinterpret_cast<const long long *>(idx)[n] : (long long)reinterpret_cast<const int *>(idx)[n];
}

// the forward's expressions, shared with the backward so that its gate is the forward's
template <typename A> __device__ __forceinline__ A xhat_of(A x, A mean, A rstd) { return (x - mean) * rstd; }
template <typename A> __device__ __forceinline__ A z_of(A xhat, A w, A b) { return fma_of(xhat, w, b); }

// ---- statistics --------------------------------------------------------------------------------------------------------
// A workgroup owns one tile of kStatTile elements of one (image, group) block, which is contiguous in NCHW: the tile's
// mean, then its sum of squared deviations from that mean, from registers.  tiles == 1: mean and rstd; otherwise the
// partials -> ws[(block * tiles + tile) * 2 + {0, 1}].
template <typename T>
__global__ __launch_bounds__(kThreads) void stat_kernel(const T *__restrict__ x, typename Acc<T>::type *__restrict__ ws,
                                                        typename Acc<T>::type *__restrict__ mean,
                                                        typename Acc<T>::type *__restrict__ rstd, const long long L,
                                                        const int tiles, const typename Acc<T>::type eps)
{
    typedef typename Acc<T>::type A;
    __shared__ A red[kWaves];
    const long long blk = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles, tid = threadIdx.x;
    const long long start = (long long)tile * kStatTile;
    const int cnt = (int)(L - start < kStatTile ? L - start : kStatTile);
    const T *p = x + blk * L + start;
    A v[kStatPer];
    A sum = (A)0;
#pragma unroll
    for (int j = 0; j < kStatPer; ++j) {
        const int i = j * kThreads + tid;
        v[j] = i < cnt ? (A)to_acc(p[i]) : (A)0;
        sum += v[j];
    }
    const A m = block_sum<kWaves>(sum, red) / (A)cnt;
    A dev = (A)0;
#pragma unroll
    for (int j = 0; j < kStatPer; ++j) {
        const A d = v[j] - m;
        if (j * kThreads + tid < cnt) dev = fma_of(d, d, dev);
    }
    const A m2 = block_sum<kWaves>(dev, red);
    if (tid == 0) {
        if (tiles == 1) {
            mean[blk] = m;
            rstd[blk] = rsqrt_of(m2 / (A)L + eps);
        } else {
            ws[(blk * tiles + tile) * 2] = m;
            ws[(blk * tiles + tile) * 2 + 1] = m2;
        }
    }
}

// One wave per (image, group): mean = sum(cnt_i * mean_i) / L, M2 = sum(M2_i + cnt_i * (mean_i - mean)^2), each a
// lane-strided loop over the tiles and a butterfly.
template <typename A>
__global__ __launch_bounds__(kThreads) void stat_combine_kernel(const A *__restrict__ ws, A *__restrict__ mean,
                                                                A *__restrict__ rstd, const long long blocks,
                                                                const long long L, const int tiles, const A eps)
{
    const long long blk = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (blk >= blocks) return;
    const A *wp = ws + blk * tiles * 2;
    const int last = (int)(L - (long long)(tiles - 1) * kStatTile);
    A s = (A)0;
    for (int i = lane; i < tiles; i += 64) s = fma_of((A)(i == tiles - 1 ? last : kStatTile), wp[2 * i], s);
    const A m = wave_sum(s) / (A)L;
    A q = (A)0;
    for (int i = lane; i < tiles; i += 64) {
        const A d = wp[2 * i] - m;
        q += fma_of((A)(i == tiles - 1 ? last : kStatTile) * d, d, wp[2 * i + 1]);
    }
    q = wave_sum(q);
    if (lane == 0) {
        mean[blk] = m;
        rstd[blk] = rsqrt_of(q / (A)L + eps);
    }
}

// ---- apply -------------------------------------------------------------------------------------------------------------
// A workgroup owns (image, kTC channels of the C + E, kTP destination pixels).  Lanes map to pixels: a wave reads one
// channel's row segment of x at src(d) (neighbouring d share or neighbour a source pixel), of skip and of extra, all
// pixel-contiguous in NCHW.  The tile goes through LDS -- rows of kTC + 1 values, so that a wave's column write and its row
// read both touch every bank once -- and leaves as channel-contiguous rows of out.
template <typename T>
__global__ __launch_bounds__(kThreads) void apply_kernel(const T *__restrict__ x, const void *__restrict__ weight,
                                                         const void *__restrict__ bias,
                                                         const typename Acc<T>::type *__restrict__ mean,
                                                         const typename Acc<T>::type *__restrict__ rstd,
                                                         const T *__restrict__ skip, const void *__restrict__ sidx,
                                                         const int is64, const void *__restrict__ extra,
                                                         void *__restrict__ out, const mhstage_shape s, const int pwide,
                                                         const int ewide, const int owide, const int ptiles, const int ctiles)
{
    typedef typename Acc<T>::type A;
    __shared__ A tile[kTP][kTC + 1];
    const int CT = s.C + s.E, P = s.H * s.W, p = s.h * s.w, cpg = s.C / s.G;
    long long b = blockIdx.x;
    const int pt = (int)(b % ptiles);
    b /= ptiles;
    const int ct = (int)(b % ctiles);
    const long long n = b / ctiles;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = pt * kTP + lane;
    const int dd = d < P ? d : P - 1;       // a pixel past the end repeats the last one: computed, never stored
    const int so = src_index(dd / s.W, s.h, s.H) * s.w + src_index(dd % s.W, s.w, s.W);
    const long long f = skip ? index_at(sidx, is64, n) : 0;
    for (int k = wave; k < kTC; k += kWaves) {
        const int c = ct * kTC + k;
        if (c >= CT) break;
        A v;
        if (c < s.C) {
            const int g = c / cpg;
            const A xh = xhat_of((A)to_acc(x[(n * s.C + c) * p + so]), mean[n * s.G + g], rstd[n * s.G + g]);
            const A z = z_of(xh, ld<T>(weight, c, pwide), ld<T>(bias, c, pwide));
            v = z > (A)0 ? z : (z == z ? (A)0 : z);
            if (skip) v += (A)to_acc(skip[(f * s.C + c) * P + dd]);
        } else {
            v = ld<T>(extra, (n * s.E + (c - s.C)) * P + dd, ewide);
        }
        tile[lane][k] = v;
    }
    __syncthreads();
    const int nc = min(kTC, CT - ct * kTC), np = min(kTP, P - pt * kTP);
    const long long base = (n * P + (long long)pt * kTP) * CT + ct * kTC;
    for (int i = tid; i < np * nc; i += kThreads) {
        const int pp = i / nc, k = i - pp * nc;
        st<T>(out, base + (long long)pp * CT + k, tile[pp][k], owide);
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
// Pass 1.  A workgroup owns (image, kBC channels, kBwdPixels source pixels); a wave takes a channel at a time and a lane
// kBP source pixels.  g = grad_out over the pixel's destination range, rows outer, columns inner; dy = g where z > 0.
// The tile's sums of dy and of dy * xhat: over a lane's pixels in ascending order, then a butterfly
// -> ws[((n * C + c) * stiles + tile) * 2 + {0, 1}].
template <typename T>
__global__ __launch_bounds__(kThreads) void bwd_gate_kernel(const T *__restrict__ x, const void *__restrict__ weight,
                                                            const void *__restrict__ bias,
                                                            const typename Acc<T>::type *__restrict__ mean,
                                                            const typename Acc<T>::type *__restrict__ rstd,
                                                            const void *__restrict__ gout, const long long gs_n,
                                                            const long long gs_c, const long long gs_y, const long long gs_x,
                                                            typename Acc<T>::type *__restrict__ dy,
                                                            typename Acc<T>::type *__restrict__ ws, const mhstage_shape s,
                                                            const int pwide, const int owide, const int stiles,
                                                            const int ctiles)
{
    typedef typename Acc<T>::type A;
    const int p = s.h * s.w, cpg = s.C / s.G;
    long long b = blockIdx.x;
    const int tile = (int)(b % stiles);
    b /= stiles;
    const int ct = (int)(b % ctiles);
    const long long n = b / ctiles;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int y0[kBP], y1[kBP], x0[kBP], x1[kBP], at[kBP];
#pragma unroll
    for (int j = 0; j < kBP; ++j) {
        const int sp = tile * kBwdPixels + j * 64 + lane;
        at[j] = sp;
        if (sp < p) {
            const int ys = sp / s.w, xs = sp - ys * s.w;
            y0[j] = first_dest(ys, s.h, s.H);
            y1[j] = ys + 1 < s.h ? first_dest(ys + 1, s.h, s.H) : s.H;
            x0[j] = first_dest(xs, s.w, s.W);
            x1[j] = xs + 1 < s.w ? first_dest(xs + 1, s.w, s.W) : s.W;
        } else {
            y0[j] = y1[j] = x0[j] = x1[j] = 0;
        }
    }
    for (int k = wave; k < kBC; k += kWaves) {
        const int c = ct * kBC + k;
        if (c >= s.C) break;
        const int g = c / cpg;
        const A mu = mean[n * s.G + g], rs = rstd[n * s.G + g];
        const A wv = ld<T>(weight, c, pwide), bv = ld<T>(bias, c, pwide);
        const long long row = (n * s.C + c) * p, gbase = n * gs_n + c * gs_c;
        A a1 = (A)0, a2 = (A)0;
#pragma unroll
        for (int j = 0; j < kBP; ++j) {
            if (at[j] >= p) continue;
            A gsum = (A)0;
            for (int yy = y0[j]; yy < y1[j]; ++yy)
                for (int xx = x0[j]; xx < x1[j]; ++xx) gsum += ld<T>(gout, gbase + yy * gs_y + xx * gs_x, owide);
            const A xh = xhat_of((A)to_acc(x[row + at[j]]), mu, rs);
            const A dv = z_of(xh, wv, bv) > (A)0 ? gsum : (A)0;
            dy[row + at[j]] = dv;
            a1 += dv;
            a2 = fma_of(dv, xh, a2);
        }
        a1 = wave_sum(a1);
        a2 = wave_sum(a2);
        if (lane == 0) {
            A *dst = ws + ((n * s.C + c) * stiles + tile) * 2;
            dst[0] = a1;
            dst[1] = a2;
        }
    }
}

// One wave per (image, group): each channel's tiles (a lane-strided loop and a butterfly) -> nc[(n * C + c) * 2 + {0, 1}]
// = (sum of dy, sum of dy * xhat), and over the group's channels in ascending order S1, S2 -> gs[(n * G + g) * 2 + {0, 1}].
template <typename T>
__global__ __launch_bounds__(kThreads) void bwd_combine_kernel(const typename Acc<T>::type *__restrict__ ws,
                                                               const void *__restrict__ weight,
                                                               typename Acc<T>::type *__restrict__ nc,
                                                               typename Acc<T>::type *__restrict__ gs, const long long blocks,
                                                               const int C, const int G, const int stiles, const int pwide)
{
    typedef typename Acc<T>::type A;
    const long long blk = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (blk >= blocks) return;
    const int cpg = C / G, g = (int)(blk % G);
    const long long n = blk / G;
    A s1 = (A)0, s2 = (A)0;
    for (int k = 0; k < cpg; ++k) {
        const int c = g * cpg + k;
        const A *wp = ws + (n * C + c) * stiles * 2;
        A a1 = (A)0, a2 = (A)0;
        for (int i = lane; i < stiles; i += 64) {
            a1 += wp[2 * i];
            a2 += wp[2 * i + 1];
        }
        a1 = wave_sum(a1);
        a2 = wave_sum(a2);
        if (lane == 0) {
            nc[(n * C + c) * 2] = a1;
            nc[(n * C + c) * 2 + 1] = a2;
        }
        const A wv = ld<T>(weight, c, pwide);
        s1 = fma_of(wv, a1, s1);
        s2 = fma_of(wv, a2, s2);
    }
    if (lane == 0) {
        gs[blk * 2] = s1;
        gs[blk * 2 + 1] = s2;
    }
}

// Pass 2: grad_x = rstd * (weight * dy - S1 / m - xhat * S2 / m), elementwise over (row = n * C + c, pixels); a thread
// reads dy[i] before it writes gx[i], so the two may be one buffer.
template <typename T>
__global__ __launch_bounds__(kThreads) void bwd_gx_kernel(const T *__restrict__ x, const void *__restrict__ weight,
                                                          const typename Acc<T>::type *__restrict__ mean,
                                                          const typename Acc<T>::type *__restrict__ rstd,
                                                          const typename Acc<T>::type *__restrict__ gs,
                                                          const typename Acc<T>::type *dy, T *gx, const int C, const int G,
                                                          const int p, const int ptiles, const int pwide)
{
    typedef typename Acc<T>::type A;
    const long long row = blockIdx.x / ptiles;
    const int pt = blockIdx.x % ptiles, cpg = C / G;
    const int c = (int)(row % C);
    const long long ng = row / C * G + c / cpg;
    const A mu = mean[ng], rs = rstd[ng], wv = ld<T>(weight, c, pwide);
    const A m = (A)cpg * (A)p;
    const A k1 = gs[ng * 2] / m, k2 = gs[ng * 2 + 1] / m;
#pragma unroll
    for (int j = 0; j < kGxPer; ++j) {
        const int i = (pt * kGxPer + j) * kThreads + threadIdx.x;
        if (i < p) {
            const A xh = xhat_of((A)to_acc(x[row * p + i]), mu, rs);
            from_acc(gx[row * p + i], rs * ((wv * dy[row * p + i] - k1) - xh * k2));
        }
    }
}

// grad_weight and grad_bias: one wave per channel, the images lane-strided and a butterfly
template <typename T>
__global__ __launch_bounds__(kThreads) void bwd_params_kernel(const typename Acc<T>::type *__restrict__ nc, void *gw, void *gb,
                                                              const int N, const int C, const int pwide)
{
    typedef typename Acc<T>::type A;
    const int c = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= C) return;
    A a1 = (A)0, a2 = (A)0;
    for (int n = lane; n < N; n += 64) {
        a1 += nc[((long long)n * C + c) * 2];
        a2 += nc[((long long)n * C + c) * 2 + 1];
    }
    a1 = wave_sum(a1);
    a2 = wave_sum(a2);
    if (lane == 0) {
        if (gb) st<T>(gb, c, a1, pwide);
        if (gw) st<T>(gw, c, a2, pwide);
    }
}

// grad_skip[f, c, d]: the images in ascending order, those with skip_index[n] == f added.  A thread per element, pixels
// fastest (skip's own NCHW order).
template <typename T>
__global__ __launch_bounds__(kThreads) void bwd_skip_kernel(const void *__restrict__ gout, const long long gs_n,
                                                            const long long gs_c, const long long gs_p,
                                                            const void *__restrict__ sidx, const int is64,
                                                            T *__restrict__ gskip, const int N, const int C, const int P,
                                                            const int ptiles, const int owide)
{
    typedef typename Acc<T>::type A;
    const long long row = blockIdx.x / ptiles;      // f * C + c
    const int d = (blockIdx.x % ptiles) * kThreads + threadIdx.x;
    if (d >= P) return;
    const long long f = row / C;
    const int c = (int)(row % C);
    A acc = (A)0;
    for (int n = 0; n < N; ++n)
        if (index_at(sidx, is64, n) == f) acc += ld<T>(gout, n * gs_n + c * gs_c + d * gs_p, owide);
    from_acc(gskip[row * P + d], acc);
}

// ---- host --------------------------------------------------------------------------------------------------------------
int check_shape(const mhstage_shape *s, bool with_skip)
{
    if (!s) return err.fail("null pointer: shape");
    if (s->N < 0 || s->E < 0 || s->C <= 0 || s->G <= 0 || s->h <= 0 || s->w <= 0 || s->H <= 0 || s->W <= 0)
        return err.fail("sizes must be positive (N and E may be 0)");
    if (with_skip && s->F <= 0) return err.fail("sizes must be positive: F = %lld beside a skip", s->F);
    if (s->C % s->G != 0) return err.fail("C = %lld channels are not a multiple of the G = %lld groups", s->C, s->G);
    if ((long long)s->h * s->w > 0x7fffffffLL) return err.fail("h * w = %lld does not fit 31 bits", (long long)s->h * s->w);
    if ((long long)s->H * s->W > 0x7fffffffLL) return err.fail("H * W = %lld does not fit 31 bits", (long long)s->H * s->W);
    if ((long long)s->C + s->E > 0x7fffffffLL) return err.fail("C + E = %lld does not fit 31 bits", (long long)s->C + s->E);
    if ((long long)(s->C / s->G) * s->h * s->w > 0x7fffffffLL)
        return err.fail("a group block of %lld elements does not fit 31 bits", (long long)(s->C / s->G) * s->h * s->w);
    return MHSTAGE_OK;
}

int check_types(int dtype, int param_wide, int extra_wide, int out_wide)
{
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (((param_wide | extra_wide | out_wide) & ~1) != 0) return err.fail("a wide flag must be 0 or 1");
    if ((param_wide || extra_wide || out_wide) && elem_size(dtype) != 2)
        return err.fail("a wide (float32) tensor goes beside a 16-bit dtype only, not beside dtype code %lld", dtype);
    return MHSTAGE_OK;
}

int stat_tiles(const mhstage_shape &s) { return (int)cdiv((long long)(s.C / s.G) * s.h * s.w, kStatTile); }
int bwd_tiles(const mhstage_shape &s) { return (int)cdiv((long long)s.h * s.w, kBwdPixels); }

template <typename T>
int launch_forward(int pwide, int ewide, int owide, const void *x, const void *weight, const void *bias, double eps,
                   const void *skip, const void *sidx, int is64, const void *extra, const mhstage_shape &s, void *ws,
                   void *mean, void *rstd, void *out, hipStream_t st)
{
    typedef typename Acc<T>::type A;
    const long long L = (long long)(s.C / s.G) * s.h * s.w, blocks = (long long)s.N * s.G;
    const int tiles = stat_tiles(s);
    const int ptiles = (int)cdiv((long long)s.H * s.W, kTP), ctiles = (int)cdiv((long long)s.C + s.E, kTC);
    unsigned g1, g2, g3;
    if (err.grid_of(blocks * tiles, &g1) || err.grid_of(cdiv(blocks, kWaves), &g2) || err.grid_of((long long)s.N * ctiles * ptiles, &g3))
        return MHSTAGE_ERR_ARGUMENT;
    hipLaunchKernelGGL((stat_kernel<T>), dim3(g1), dim3(kThreads), 0, st, (const T *)x, (A *)ws, (A *)mean, (A *)rstd, L, tiles,
                       (A)eps);
    if (tiles > 1)
        hipLaunchKernelGGL((stat_combine_kernel<A>), dim3(g2), dim3(kThreads), 0, st, (const A *)ws, (A *)mean, (A *)rstd,
                           blocks, L, tiles, (A)eps);
    hipLaunchKernelGGL((apply_kernel<T>), dim3(g3), dim3(kThreads), 0, st, (const T *)x, weight, bias, (const A *)mean,
                       (const A *)rstd, (const T *)skip, sidx, is64, extra, out, s, pwide, ewide, owide, ptiles, ctiles);
    return err.check_launch("mhstage_forward");
}

template <typename T>
int launch_backward(int grads, int pwide, int owide, const void *x, const void *weight, const void *bias, const void *mean,
                    const void *rstd, const void *sidx, int is64, const void *gout, int layout, const mhstage_shape &s,
                    void *ws, void *dy, void *gx, void *gw, void *gb, void *gskip, hipStream_t st)
{
    typedef typename Acc<T>::type A;
    const long long CT = (long long)s.C + s.E, P = (long long)s.H * s.W, p = (long long)s.h * s.w;
    const long long gs_n = CT * P, gs_c = layout ? 1 : P, gs_x = layout ? CT : 1, gs_y = gs_x * s.W;
    if (grads & (MHSTAGE_GRAD_X | MHSTAGE_GRAD_WEIGHT | MHSTAGE_GRAD_BIAS)) {
        const int stiles = bwd_tiles(s), ctiles = (int)cdiv(s.C, kBC), ptiles = (int)cdiv(p, kThreads * kGxPer);
        A *part = (A *)ws, *nc = part + (long long)s.N * s.C * stiles * 2, *gsum = nc + (long long)s.N * s.C * 2;
        unsigned g1, g2, g3, g4;
        if (err.grid_of((long long)s.N * ctiles * stiles, &g1) || err.grid_of(cdiv((long long)s.N * s.G, kWaves), &g2) ||
            err.grid_of((long long)s.N * s.C * ptiles, &g3) || err.grid_of(cdiv(s.C, kWaves), &g4))
            return MHSTAGE_ERR_ARGUMENT;
        hipLaunchKernelGGL((bwd_gate_kernel<T>), dim3(g1), dim3(kThreads), 0, st, (const T *)x, weight, bias, (const A *)mean,
                           (const A *)rstd, gout, gs_n, gs_c, gs_y, gs_x, (A *)dy, part, s, pwide, owide, stiles, ctiles);
        hipLaunchKernelGGL((bwd_combine_kernel<T>), dim3(g2), dim3(kThreads), 0, st, (const A *)part, weight, nc, gsum,
                           (long long)s.N * s.G, s.C, s.G, stiles, pwide);
        if (grads & MHSTAGE_GRAD_X)
            hipLaunchKernelGGL((bwd_gx_kernel<T>), dim3(g3), dim3(kThreads), 0, st, (const T *)x, weight, (const A *)mean,
                               (const A *)rstd, (const A *)gsum, (const A *)dy, (T *)gx, s.C, s.G, (int)p, ptiles, pwide);
        if (grads & (MHSTAGE_GRAD_WEIGHT | MHSTAGE_GRAD_BIAS))
            hipLaunchKernelGGL((bwd_params_kernel<T>), dim3(g4), dim3(kThreads), 0, st, (const A *)nc,
                               (grads & MHSTAGE_GRAD_WEIGHT) ? gw : nullptr, (grads & MHSTAGE_GRAD_BIAS) ? gb : nullptr, s.N,
                               s.C, pwide);
    }
    if (grads & MHSTAGE_GRAD_SKIP) {
        const int ptiles = (int)cdiv(P, kThreads);
        unsigned g5;
        if (err.grid_of((long long)s.F * s.C * ptiles, &g5)) return MHSTAGE_ERR_ARGUMENT;
        hipLaunchKernelGGL((bwd_skip_kernel<T>), dim3(g5), dim3(kThreads), 0, st, gout, gs_n, gs_c, gs_x, sidx, is64,
                           (T *)gskip, s.N, s.C, (int)P, ptiles, owide);
    }
    return err.check_launch("mhstage_backward");
}

}  // namespace mhstage

using namespace mhstage;

extern "C" {

int mhstage_version(void) { return MHSTAGE_ABI_VERSION; }

const char *mhstage_last_error(void) { return err.msg; }

int mhstage_tile(int which)
{
    switch (which) {
    case MHSTAGE_TILE_STAT: return kStatTile;
    case MHSTAGE_TILE_APPLY_PIXELS: return kTP;
    case MHSTAGE_TILE_APPLY_CHANNELS: return kTC;
    case MHSTAGE_TILE_BWD_PIXELS: return kBwdPixels;
    default: return -1;
    }
}

long long mhstage_workspace_bytes(int dtype, const mhstage_shape *shape)
{
    err.clear();
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (check_shape(shape, false) != MHSTAGE_OK) return MHSTAGE_ERR_ARGUMENT;
    const mhstage_shape &s = *shape;
    const long long fwd = (long long)s.N * s.G * stat_tiles(s) * 2;
    const long long bwd = (long long)s.N * s.C * bwd_tiles(s) * 2 + (long long)s.N * s.C * 2 + (long long)s.N * s.G * 2;
    const long long bytes = (fwd > bwd ? fwd : bwd) * acc_size(dtype);
    return (bytes + 255) / 256 * 256;
}

int mhstage_forward(int dtype, int param_wide, int extra_wide, int out_wide, const void *x, const void *weight,
                    const void *bias, double eps, const void *skip, const void *skip_index, int index_is64,
                    const void *extra, const mhstage_shape *shape, void *workspace, void *mean, void *rstd, void *out,
                    void *stream)
{
    err.clear();
    if (check_types(dtype, param_wide, extra_wide, out_wide) != MHSTAGE_OK || check_shape(shape, skip != nullptr) != MHSTAGE_OK)
        return MHSTAGE_ERR_ARGUMENT;
    const mhstage_shape &s = *shape;
    if (!skip && !extra && (s.H != s.h || s.W != s.w))
        return err.fail("without skip and extra the output map is the input's: H, W must be h, w");
    if (!skip && skip_index) return err.fail("skip_index without skip");
    if (skip && !skip_index && s.F != s.N) return err.fail("without skip_index F = %lld must equal N = %lld", s.F, s.N);
    if ((s.E > 0) != (extra != nullptr)) return err.fail("null pointer: extra must be given exactly when E = %lld > 0", s.E);
    if (s.N == 0) return MHSTAGE_OK;
    if (!x || !weight || !bias || !workspace || !mean || !rstd || !out)
        return err.fail("null pointer: x, weight, bias, workspace, mean, rstd and out are required");
    hipStream_t st = (hipStream_t)stream;
    return dispatch(dtype, [&](auto t) {
        return launch_forward<type_of<decltype(t)>>(param_wide, extra_wide, out_wide, x, weight, bias, eps, skip, skip_index,
                                                    index_is64, extra, s, workspace, mean, rstd, out, st);
    });
}

int mhstage_backward(int grads, int dtype, int param_wide, int out_wide, const void *x, const void *weight,
                     const void *bias, const void *mean, const void *rstd, const void *skip_index, int index_is64,
                     const void *grad_out, int grad_out_layout, const mhstage_shape *shape, void *workspace, void *dy,
                     void *grad_x, void *grad_weight, void *grad_bias, void *grad_skip, void *stream)
{
    err.clear();
    const int all = MHSTAGE_GRAD_X | MHSTAGE_GRAD_WEIGHT | MHSTAGE_GRAD_BIAS | MHSTAGE_GRAD_SKIP;
    if (check_types(dtype, param_wide, 0, out_wide) != MHSTAGE_OK) return MHSTAGE_ERR_ARGUMENT;
    if (grads < 0 || grads > all) return err.fail("grads = %lld is not a mask of the MHSTAGE_GRAD_* bits", grads);
    if (grad_out_layout != 0 && grad_out_layout != 1) return err.fail("grad_out_layout = %lld must be 0 (NCHW) or 1 (channels-last)", grad_out_layout);
    if (check_shape(shape, (grads & MHSTAGE_GRAD_SKIP) != 0) != MHSTAGE_OK) return MHSTAGE_ERR_ARGUMENT;
    const mhstage_shape &s = *shape;
    if ((grads & MHSTAGE_GRAD_SKIP) && !skip_index && s.F != s.N)
        return err.fail("without skip_index F = %lld must equal N = %lld", s.F, s.N);
    if (grads == 0 || (s.N == 0 && !(grads & MHSTAGE_GRAD_SKIP))) return MHSTAGE_OK;
    if (!grad_out && s.N > 0) return err.fail("null pointer: grad_out is required");
    if (grads & (all & ~MHSTAGE_GRAD_SKIP)) {
        if (!x || !weight || !bias || !mean || !rstd || !workspace || !dy)
            return err.fail("null pointer: x, weight, bias, mean, rstd, workspace and dy are required");
        if (((grads & MHSTAGE_GRAD_X) && !grad_x) || ((grads & MHSTAGE_GRAD_WEIGHT) && !grad_weight) ||
            ((grads & MHSTAGE_GRAD_BIAS) && !grad_bias))
            return err.fail("null pointer: a gradient named in grads = %lld has no buffer", grads);
        if (grad_x && dy == grad_x && elem_size(dtype) == 2) return err.fail("grad_x may alias dy for MHSTAGE_F32 and MHSTAGE_F64 only");
    }
    if ((grads & MHSTAGE_GRAD_SKIP) && !grad_skip) return err.fail("null pointer: a gradient named in grads = %lld has no buffer", grads);
    if (s.N == 0) grads &= MHSTAGE_GRAD_SKIP;      // no image: grad_skip is all zeros, the parameters' sums too (the caller's)
    hipStream_t st = (hipStream_t)stream;
    return dispatch(dtype, [&](auto t) {
        return launch_backward<type_of<decltype(t)>>(grads, param_wide, out_wide, x, weight, bias, mean, rstd, skip_index,
                                                     index_is64, grad_out, grad_out_layout, s, workspace, dy, grad_x, grad_weight,
                                                     grad_bias, grad_skip, st);
    });
}

}  // extern "C"
