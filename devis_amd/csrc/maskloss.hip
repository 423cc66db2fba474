// maskloss.hip -- the mask loss (include/maskloss.h): bilinear resampling of the logit maps to the
// target resolution, sigmoid focal loss and dice loss in one pass over the target pixels plus a fixed-order combine, and the
// backward as a gather over each source pixel's footprint.  gfx950, wave64, plain HIP, fp32 arithmetic (fp64 for doubles);
// no atomics: every sum has a fixed order.
//
// The kernels are templates of the storage type of src alone.  The target kind and how gamma is applied are kernel
// arguments: wave-uniform branches, not compile-time variants.
#include "op_common.h"       // (fp contraction off)
#include "maskloss.h"

namespace maskloss {

using namespace devis;

static_assert(MASKLOSS_OK == kOk && MASKLOSS_ERR_ARGUMENT == kErrArgument && MASKLOSS_ERR_HIP == kErrHip, "status codes");
static_assert(MASKLOSS_F32 == kF32 && MASKLOSS_F64 == kF64 && MASKLOSS_BF16 == kBF16 && MASKLOSS_F16 == kF16, "dtype codes");

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = 16;                        // forward: consecutive destination pixels per lane (one 16-byte load of U8)
constexpr int kFwdTile = kThreads * kPer;
constexpr int kSrcCap = 4096;                   // forward: source elements kept in LDS
constexpr int kBY = 8, kBX = 32;                // backward: source rows x columns per workgroup, one pixel per lane
constexpr int kChunk = 4096;                    // backward: destination pixels of g held in LDS at a time
static_assert(kBY * kBX == kThreads, "one source pixel per lane");

enum { kGammaZero = 0, kGammaOne = 1, kGammaTwo = 2, kGammaPow = 3 };

thread_local Status err;     // maskloss_last_error()

// ---- the resampling rule (include/maskloss.h), per axis, in the arithmetic type ---------------------------------------
template <typename A> struct Tap {
    int i0, i1;
    A l0, l1;
};

template <typename A> __device__ __forceinline__ Tap<A> tap_of(int d, int in, int out)
{
    const A scale = (A)in / (A)out;
    A r = scale * ((A)d + (A)0.5) - (A)0.5;
    r = r > (A)0 ? r : (A)0;
    Tap<A> t;
    t.i0 = (int)r;
    if (t.i0 > in - 1) t.i0 = in - 1;       // (never taken for a finite rule; keeps every index inside the map)
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = r - (A)t.i0;
    t.l0 = (A)1 - t.l1;
    return t;
}

// the first d in [0, out] whose i0 is >= s (out when there is none); i0 is monotone in d
template <typename A> __device__ __forceinline__ int first_ge(int s, int in, int out)
{
    if (s <= 0) return 0;
    A est = ((A)s + (A)0.5) * ((A)out / (A)in) - (A)0.5;
    int d = est < (A)0 ? 0 : (est > (A)out ? out : (int)est);
    while (d > 0 && tap_of<A>(d - 1, in, out).i0 >= s) --d;
    while (d < out && tap_of<A>(d, in, out).i0 < s) ++d;
    return d;
}

// the destination indices whose taps contain source index s: [foot_lo, foot_hi)
template <typename A> __device__ __forceinline__ int foot_lo(int s, int in, int out) { return first_ge<A>(s - 1, in, out); }
template <typename A> __device__ __forceinline__ int foot_hi(int s, int in, int out)
{
    return s + 1 <= in - 1 ? first_ge<A>(s + 1, in, out) : out;
}

// the weight of source index s in the taps of destination index d
template <typename A> __device__ __forceinline__ A weight_of(int d, int s, int in, int out)
{
    const Tap<A> t = tap_of<A>(d, in, out);
    return (t.i0 == s ? t.l0 : (A)0) + (t.i1 == s ? t.l1 : (A)0);
}

// ---- one pixel ------------------------------------------------------------------------------------------------------
template <typename A> struct Pixel {
    A p, ce, m;     // sigmoid, cross entropy, 1 - p_t
};

template <typename A> __device__ __forceinline__ Pixel<A> pixel_of(A x, A t)
{
    Pixel<A> q;
    const A e = exp_of(-(x < (A)0 ? -x : x));
    const A inv = (A)1 / ((A)1 + e);
    q.p = x >= (A)0 ? inv : e * inv;
    q.ce = (x > (A)0 ? x : (x == x ? (A)0 : x)) - x * t + log1p_of(e);
    const A pt = q.p * t + ((A)1 - q.p) * ((A)1 - t);
    q.m = (A)1 - pt;
    return q;
}

// m^gamma
template <typename A> __device__ __forceinline__ A mod_of(A m, A gamma, int gm)
{
    if (gm == kGammaTwo) return m * m;
    if (gm == kGammaOne) return m;
    if (gm == kGammaZero) return (A)1;
    return pow_of(m > (A)0 ? m : (A)0, gamma);
}

// gamma * m^(gamma-1)
template <typename A> __device__ __forceinline__ A dmod_of(A m, A gamma, int gm)
{
    if (gm == kGammaTwo) return (A)2 * m;
    if (gm == kGammaOne) return (A)1;
    if (gm == kGammaZero) return (A)0;
    return gamma * pow_of(m > (A)0 ? m : (A)0, gamma - (A)1);
}

template <typename A> __device__ __forceinline__ A alpha_of(A t, A alpha)
{
    return alpha >= (A)0 ? alpha * t + ((A)1 - alpha) * ((A)1 - t) : (A)1;
}

template <typename T> __device__ __forceinline__ typename Acc<T>::type target_at(const void *tgt, long long i, int tk)
{
    typedef typename Acc<T>::type A;
    if (tk == MASKLOSS_TARGET_U8) return reinterpret_cast<const unsigned char *>(tgt)[i] ? (A)1 : (A)0;
    if (tk == MASKLOSS_TARGET_F32) return (A) reinterpret_cast<const float *>(tgt)[i];
    return (A)to_acc(reinterpret_cast<const T *>(tgt)[i]);
}

template <typename A> __device__ __forceinline__ void finish(A fsum, A a, A b, A c, int P, A *focal, A *dice, A *sums)
{
    *focal = fsum / (A)P;
    *dice = (A)1 - ((A)2 * a + (A)1) / (b + c + (A)1);
    sums[0] = a;
    sums[1] = b;
    sums[2] = c;
}

// ---- forward --------------------------------------------------------------------------------------------------------
// A workgroup owns kFwdTile consecutive destination pixels of one instance, a lane kPer consecutive ones of them.  The
// source rows the tile's taps touch are staged in LDS in the arithmetic type when they fit kSrcCap elements (they do unless
// the map is downsampled steeply), else read from memory.  A lane sums its pixels ascending; lanes by a butterfly, waves
// ascending.  tiles == 1: the instance's results; otherwise the four partials -> ws[(n * tiles + tile) * 4 + {0..3}].
template <typename T>
__global__ __launch_bounds__(kThreads) void forward_kernel(const T *__restrict__ src, const void *__restrict__ tgt, const int tk,
                                                           typename Acc<T>::type *__restrict__ ws,
                                                           typename Acc<T>::type *__restrict__ focal,
                                                           typename Acc<T>::type *__restrict__ dice,
                                                           typename Acc<T>::type *__restrict__ sums, const maskloss_shape s,
                                                           const int tiles, const typename Acc<T>::type alpha,
                                                           const typename Acc<T>::type gamma, const int gm)
{
    typedef typename Acc<T>::type A;
    __shared__ A rows[kSrcCap];
    __shared__ A red[4][kWaves];
    const long long n = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles, tid = threadIdx.x;
    const int P = s.H * s.W, p = s.h * s.w;
    const int base = tile * kFwdTile;
    const int end = P - base < kFwdTile ? P : base + kFwdTile;
    const T *sp = src + n * p;
    // the source rows of the tile's first and last destination row
    const int r0 = tap_of<A>(base / s.W, s.h, s.H).i0, r1 = tap_of<A>((end - 1) / s.W, s.h, s.H).i1;
    const bool staged = (long long)(r1 - r0 + 1) * s.w <= kSrcCap;
    if (staged) {
        const int cnt = (r1 - r0 + 1) * s.w;
        for (int i = tid; i < cnt; i += kThreads) rows[i] = (A)to_acc(sp[r0 * s.w + i]);
        __syncthreads();
    }
    A fs = (A)0, sa = (A)0, sb = (A)0, sc = (A)0;
    const int d0 = base + tid * kPer;
    if (d0 < end) {
        const long long at = n * P + d0;
        const bool vec = tk == MASKLOSS_TARGET_U8 && d0 + kPer <= end &&
                         ((reinterpret_cast<unsigned long long>(tgt) + (unsigned long long)at) & 15ull) == 0;
        unsigned int word[4] = {0u, 0u, 0u, 0u};
        if (vec) {
            const uint4 v = *reinterpret_cast<const uint4 *>(reinterpret_cast<const unsigned char *>(tgt) + at);
            word[0] = v.x; word[1] = v.y; word[2] = v.z; word[3] = v.w;
        }
        int y = d0 / s.W, xq = d0 - y * s.W;
        Tap<A> ty = tap_of<A>(y, s.h, s.H);
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            if (d0 + j < end) {
                const Tap<A> tx = tap_of<A>(xq, s.w, s.W);
                A v00, v01, v10, v11;
                if (staged) {
                    const A *ra = rows + (ty.i0 - r0) * s.w, *rb = rows + (ty.i1 - r0) * s.w;
                    v00 = ra[tx.i0]; v01 = ra[tx.i1]; v10 = rb[tx.i0]; v11 = rb[tx.i1];
                } else {
                    const T *ra = sp + ty.i0 * s.w, *rb = sp + ty.i1 * s.w;
                    v00 = (A)to_acc(ra[tx.i0]); v01 = (A)to_acc(ra[tx.i1]);
                    v10 = (A)to_acc(rb[tx.i0]); v11 = (A)to_acc(rb[tx.i1]);
                }
                const A x = ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
                const A t = vec ? (((word[j >> 2] >> ((j & 3) * 8)) & 0xffu) ? (A)1 : (A)0) : target_at<T>(tgt, at + j, tk);
                const Pixel<A> q = pixel_of(x, t);
                fs += q.ce * mod_of(q.m, gamma, gm) * alpha_of(t, alpha);
                sa += q.p * t;
                sb += q.p;
                sc += t;
                if (++xq == s.W) {
                    xq = 0;
                    ++y;
                    if (y < s.H) ty = tap_of<A>(y, s.h, s.H);
                }
            }
        }
    }
    fs = wave_sum(fs); sa = wave_sum(sa); sb = wave_sum(sb); sc = wave_sum(sc);
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = fs; red[1][tid >> 6] = sa; red[2][tid >> 6] = sb; red[3][tid >> 6] = sc;
    }
    __syncthreads();
    if (tid == 0) {
        A v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = red[k][0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) v[k] += red[k][w];
        }
        if (tiles == 1) {
            finish(v[0], v[1], v[2], v[3], P, focal + n, dice + n, sums + n * 3);
        } else {
            A *dst = ws + (n * tiles + tile) * 4;
            dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
        }
    }
}

// One wave per instance: the tiles lane-strided in ascending order, then a butterfly.
template <typename A>
__global__ __launch_bounds__(kThreads) void combine_kernel(const A *__restrict__ ws, A *__restrict__ focal, A *__restrict__ dice,
                                                           A *__restrict__ sums, const int N, const int tiles, const int P)
{
    const long long n = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (n >= N) return;
    const A *wp = ws + n * tiles * 4;
    A v[4] = {(A)0, (A)0, (A)0, (A)0};
    for (int i = lane; i < tiles; i += 64) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += wp[4 * i + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = wave_sum(v[k]);
    if (lane == 0) finish(v[0], v[1], v[2], v[3], P, focal + n, dice + n, sums + n * 3);
}

// ---- backward -------------------------------------------------------------------------------------------------------
// A workgroup owns kBY x kBX source pixels of one instance, one per lane.  The destination region the tile's taps cover
// (the footprints of its rows times those of its columns) is walked in chunks of at most kChunk pixels, whole row segments:
// every thread computes g for its share of the chunk into LDS, then each source pixel adds, for the chunk's rows in its
// footprint ascending, (its row weight) * (the sum over the chunk's columns in its footprint, ascending, of its column
// weight * g).  The chunk shape depends on the geometry alone, so the order of every sum does too.
template <typename T>
__global__ __launch_bounds__(kThreads) void backward_kernel(const T *__restrict__ src, const void *__restrict__ tgt, const int tk,
                                                            const typename Acc<T>::type *__restrict__ sums,
                                                            const typename Acc<T>::type *__restrict__ gfocal,
                                                            const typename Acc<T>::type *__restrict__ gdice,
                                                            T *__restrict__ gsrc, const maskloss_shape s, const int tx,
                                                            const int ty, const typename Acc<T>::type alpha,
                                                            const typename Acc<T>::type gamma, const int gm)
{
    typedef typename Acc<T>::type A;
    __shared__ A g[kChunk];
    long long b = blockIdx.x;
    const int txi = (int)(b % tx);
    b /= tx;
    const int tyi = (int)(b % ty);
    const long long n = b / ty;
    const int tid = threadIdx.x;
    const int P = s.H * s.W, p = s.h * s.w;
    const int sy0 = tyi * kBY, sx0 = txi * kBX;
    const int syl = (sy0 + kBY < s.h ? sy0 + kBY : s.h) - 1, sxl = (sx0 + kBX < s.w ? sx0 + kBX : s.w) - 1;
    const int sy = sy0 + tid / kBX, sx = sx0 + tid % kBX;
    const bool valid = sy < s.h && sx < s.w;
    // the tile's destination region and this pixel's footprint inside it
    const int RY0 = foot_lo<A>(sy0, s.h, s.H), RY1 = foot_hi<A>(syl, s.h, s.H);
    const int RX0 = foot_lo<A>(sx0, s.w, s.W), RX1 = foot_hi<A>(sxl, s.w, s.W);
    int ylo = 0, yhi = 0, xlo = 0, xhi = 0;
    if (valid) {
        ylo = foot_lo<A>(sy, s.h, s.H); yhi = foot_hi<A>(sy, s.h, s.H);
        xlo = foot_lo<A>(sx, s.w, s.W); xhi = foot_hi<A>(sx, s.w, s.W);
    }
    const T *sp = src + n * p;
    const long long tbase = n * P;
    const A sA = sums[n * 3], sB = sums[n * 3 + 1], sC = sums[n * 3 + 2];
    const A den = sB + sC + (A)1, num = (A)2 * sA + (A)1;
    const A cf = gfocal[n] / (A)P, cd = gdice[n];
    const int rw = RX1 - RX0, rh = RY1 - RY0;
    A acc = (A)0;
    if (rw > 0 && rh > 0) {
        const int CC = rw < kChunk ? rw : kChunk;
        int CR = kChunk / CC;
        CR = CR < rh ? CR : rh;
        for (int cy = RY0; cy < RY1; cy += CR) {
            const int ch = RY1 - cy < CR ? RY1 - cy : CR;
            for (int cx = RX0; cx < RX1; cx += CC) {
                const int cw = RX1 - cx < CC ? RX1 - cx : CC;
                for (int i = tid; i < ch * cw; i += kThreads) {
                    const int yy = cy + i / cw, xx = cx + i % cw;
                    const Tap<A> ay = tap_of<A>(yy, s.h, s.H), ax = tap_of<A>(xx, s.w, s.W);
                    const T *ra = sp + ay.i0 * s.w, *rb = sp + ay.i1 * s.w;
                    const A v00 = (A)to_acc(ra[ax.i0]), v01 = (A)to_acc(ra[ax.i1]);
                    const A v10 = (A)to_acc(rb[ax.i0]), v11 = (A)to_acc(rb[ax.i1]);
                    const A x = ay.l0 * (ax.l0 * v00 + ax.l1 * v01) + ay.l1 * (ax.l0 * v10 + ax.l1 * v11);
                    const A t = target_at<T>(tgt, tbase + (long long)yy * s.W + xx, tk);
                    const Pixel<A> q = pixel_of(x, t);
                    const A pq = q.p * ((A)1 - q.p);
                    const A df = alpha_of(t, alpha) * ((q.p - t) * mod_of(q.m, gamma, gm) +
                                                       q.ce * dmod_of(q.m, gamma, gm) * ((A)1 - (A)2 * t) * pq);
                    const A dd = -((A)2 * t * den - num) / (den * den) * pq;
                    g[i] = cf * df + cd * dd;
                }
                __syncthreads();
                const int ya = ylo > cy ? ylo : cy, yb = yhi < cy + ch ? yhi : cy + ch;
                const int xa = xlo > cx ? xlo : cx, xb = xhi < cx + cw ? xhi : cx + cw;
                for (int dy = ya; dy < yb; ++dy) {
                    const A *gr = g + (dy - cy) * cw - cx;
                    A rs = (A)0;
                    for (int dx = xa; dx < xb; ++dx) rs += weight_of<A>(dx, sx, s.w, s.W) * gr[dx];
                    acc += weight_of<A>(dy, sy, s.h, s.H) * rs;
                }
                __syncthreads();
            }
        }
    }
    if (valid) from_acc(gsrc[n * p + sy * s.w + sx], acc);
}

// ---- host -----------------------------------------------------------------------------------------------------------
int check_shape(const maskloss_shape *s)
{
    if (!s) return err.fail("null pointer: shape");
    if (s->N < 0 || s->h <= 0 || s->w <= 0 || s->H <= 0 || s->W <= 0)
        return err.fail("sizes must be positive (N may be 0)");
    if ((long long)s->h * s->w > 0x7fffffffLL) return err.fail("h * w = %lld does not fit 31 bits", (long long)s->h * s->w);
    if ((long long)s->H * s->W > 0x7fffffffLL) return err.fail("H * W = %lld does not fit 31 bits", (long long)s->H * s->W);
    return MASKLOSS_OK;
}

int check_types(int dtype, int target_kind)
{
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (target_kind != MASKLOSS_TARGET_U8 && target_kind != MASKLOSS_TARGET_SAME && target_kind != MASKLOSS_TARGET_F32)
        return err.fail("bad target kind %lld", target_kind);
    return MASKLOSS_OK;
}

// how gamma is applied; negative on a gamma the operator refuses
int gamma_mode(double gamma)
{
    if (!(gamma >= 0.0) || gamma > 1.0e30) return err.fail("gamma must be 0, 1 or larger than 1 (and finite)");
    if (gamma == 0.0) return kGammaZero;
    if (gamma == 1.0) return kGammaOne;
    if (gamma == 2.0) return kGammaTwo;
    if (gamma < 1.0) return err.fail("gamma in (0, 1) is not supported: the derivative is unbounded at p_t = 1");
    return kGammaPow;
}

int fwd_tiles(const maskloss_shape &s) { return (int)cdiv((long long)s.H * s.W, kFwdTile); }

template <typename T>
int launch_forward(int tk, const void *src, const void *tgt, const maskloss_shape &s, double alpha, double gamma, int gm,
                   void *ws, void *focal, void *dice, void *sums, hipStream_t st)
{
    typedef typename Acc<T>::type A;
    const int tiles = fwd_tiles(s);
    unsigned g1, g2;
    if (err.grid_of((long long)s.N * tiles, &g1) || err.grid_of(cdiv(s.N, kWaves), &g2)) return MASKLOSS_ERR_ARGUMENT;
    hipLaunchKernelGGL((forward_kernel<T>), dim3(g1), dim3(kThreads), 0, st, (const T *)src, tgt, tk, (A *)ws, (A *)focal,
                       (A *)dice, (A *)sums, s, tiles, (A)alpha, (A)gamma, gm);
    if (tiles > 1)
        hipLaunchKernelGGL((combine_kernel<A>), dim3(g2), dim3(kThreads), 0, st, (const A *)ws, (A *)focal, (A *)dice,
                           (A *)sums, s.N, tiles, s.H * s.W);
    return err.check_launch("maskloss_forward");
}

template <typename T>
int launch_backward(int tk, const void *src, const void *tgt, const void *sums, const void *gf, const void *gd,
                    const maskloss_shape &s, double alpha, double gamma, int gm, void *gsrc, hipStream_t st)
{
    typedef typename Acc<T>::type A;
    const int tx = (int)cdiv(s.w, kBX), ty = (int)cdiv(s.h, kBY);
    unsigned g1;
    if (err.grid_of((long long)s.N * tx * ty, &g1)) return MASKLOSS_ERR_ARGUMENT;
    hipLaunchKernelGGL((backward_kernel<T>), dim3(g1), dim3(kThreads), 0, st, (const T *)src, tgt, tk, (const A *)sums,
                       (const A *)gf, (const A *)gd, (T *)gsrc, s, tx, ty, (A)alpha, (A)gamma, gm);
    return err.check_launch("maskloss_backward");
}

}  // namespace maskloss

using namespace maskloss;

extern "C" {

int maskloss_version(void) { return MASKLOSS_ABI_VERSION; }

const char *maskloss_last_error(void) { return err.msg; }

int maskloss_tile(int which)
{
    switch (which) {
    case MASKLOSS_TILE_FWD_PIXELS: return kFwdTile;
    case MASKLOSS_TILE_FWD_SRC: return kSrcCap;
    case MASKLOSS_TILE_BWD_ROWS: return kBY;
    case MASKLOSS_TILE_BWD_COLS: return kBX;
    case MASKLOSS_TILE_BWD_CHUNK: return kChunk;
    default: return -1;
    }
}

long long maskloss_workspace_bytes(int dtype, const maskloss_shape *shape)
{
    err.clear();
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (check_shape(shape) != MASKLOSS_OK) return MASKLOSS_ERR_ARGUMENT;
    const int tiles = fwd_tiles(*shape);
    const long long bytes = tiles > 1 ? (long long)shape->N * tiles * 4 * acc_size(dtype) : 0;
    return (bytes + 255) / 256 * 256;
}

int maskloss_forward(int dtype, int target_kind, const void *src, const void *target, const maskloss_shape *shape,
                     double alpha, double gamma, void *workspace, void *focal, void *dice, void *sums, void *stream)
{
    err.clear();
    if (check_types(dtype, target_kind) != MASKLOSS_OK || check_shape(shape) != MASKLOSS_OK) return MASKLOSS_ERR_ARGUMENT;
    const int gm = gamma_mode(gamma);
    if (gm < 0) return MASKLOSS_ERR_ARGUMENT;
    if (!(alpha == alpha)) return err.fail("alpha must be a number");
    const maskloss_shape &s = *shape;
    if (s.N == 0) return MASKLOSS_OK;
    if (!src || !target || !focal || !dice || !sums) return err.fail("null pointer: src, target, focal, dice and sums are required");
    if (!workspace && fwd_tiles(s) > 1) return err.fail("null pointer: workspace is required when an instance is more than one tile");
    hipStream_t st = (hipStream_t)stream;
    return dispatch(dtype, [&](auto t) {
        return launch_forward<type_of<decltype(t)>>(target_kind, src, target, s, alpha, gamma, gm, workspace, focal, dice, sums, st);
    });
}

int maskloss_backward(int dtype, int target_kind, const void *src, const void *target, const void *sums,
                      const void *grad_focal, const void *grad_dice, const maskloss_shape *shape, double alpha,
                      double gamma, void *grad_src, void *stream)
{
    err.clear();
    if (check_types(dtype, target_kind) != MASKLOSS_OK || check_shape(shape) != MASKLOSS_OK) return MASKLOSS_ERR_ARGUMENT;
    const int gm = gamma_mode(gamma);
    if (gm < 0) return MASKLOSS_ERR_ARGUMENT;
    if (!(alpha == alpha)) return err.fail("alpha must be a number");
    const maskloss_shape &s = *shape;
    if (s.N == 0) return MASKLOSS_OK;
    if (!src || !target || !sums || !grad_focal || !grad_dice || !grad_src)
        return err.fail("null pointer: src, target, sums, grad_focal, grad_dice and grad_src are required");
    hipStream_t st = (hipStream_t)stream;
    return dispatch(dtype, [&](auto t) {
        return launch_backward<type_of<decltype(t)>>(target_kind, src, target, sums, grad_focal, grad_dice, s, alpha, gamma, gm,
                                                     grad_src, st);
    });
}

}  // extern "C"
