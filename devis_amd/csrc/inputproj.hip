// inputproj.hip -- the GroupNorm of the encoder's input projections written as flat tokens (include/inputproj.h; DESIGN.md
// section 25), forward and backward.  gfx950, wave64, plain HIP.  Two kernel families: the statistics of a group, which is one
// contiguous run of an NCHW map (mhstage.hip's passes, for all levels in one launch and combined by Chan's formula), and the
// pixels x channels tile that turns the map into token order through LDS (the mirror image of swinends.hip's map tile).  No
// atomics, nothing is zeroed by a pass of its own: every output element is written by the launch that owns it.
#include "op_common.h"       // (fp contraction off)
#include "inputproj.h"

namespace inputproj {

using namespace devis;
using devis::normrow::aligned16;

static_assert(INPUTPROJ_OK == kOk && INPUTPROJ_ERR_ARGUMENT == kErrArgument && INPUTPROJ_ERR_HIP == kErrHip, "status codes");
static_assert(INPUTPROJ_F32 == kF32 && INPUTPROJ_BF16 == kBF16 && INPUTPROJ_F16 == kF16, "dtype codes");

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxL = INPUTPROJ_MAX_LEVELS;
constexpr int kMaxC = INPUTPROJ_MAX_CHANNELS;
constexpr int kTileP = 64;                  // pixels of a tile: one per lane on the map side
constexpr int kTileC = 64;                  // channels of a tile
constexpr int kPitch = kTileP + 1;          // floats of a tile row: odd, so that a wave's accesses along either side spread over the banks
constexpr int kRows = kTileC / kWaves;      // channel rows of a wave on the map side
constexpr int kStatChunk = 4096;            // elements of a chunk of a group's statistics: 16 per thread
constexpr int kSumChunk = 512;              // pixels of a chunk of the backward's per-channel sums
constexpr int kSumTiles = kSumChunk / kTileP;
static_assert(kTileP == 64 && kSumChunk % kTileP == 0 && kStatChunk % (kThreads * 8) == 0, "tiling");

thread_local Status err;     // inputproj_last_error()

struct Levels {
    const void *p[kMaxL];
};
struct OutLevels {
    void *p[kMaxL];
};

// What the kernels know of a call.  block0 tables are prefix sums over the levels: level l owns the workgroups
// [block0[l], block0[l + 1]) of a launch.
struct Geo {
    int N, C, G, L, cpg;
    long long S;
    int HW[kMaxL];
    long long start[kMaxL];                 // token offset of a level
    int ptiles[kMaxL];                      // pixel tiles of a level
    long long tblock0[kMaxL + 1];           // apply / grad_x: N * ptiles workgroups per level
    int schunks[kMaxL];                     // statistics chunks of a group
    long long sblock0[kMaxL + 1];           // statistics: N * G * schunks workgroups per level
    int bchunks[kMaxL];                     // pixel chunks of the backward's sums
    long long bblock0[kMaxL + 1];           // sums: N * bchunks workgroups per level
};

__device__ __forceinline__ int level_of(const long long *block0, int L, long long b)
{
    int l = 0;
    while (l + 1 < L && b >= block0[l + 1]) ++l;
    return l;
}

// ---- V consecutive elements ------------------------------------------------------------------------------------------------
template <typename T, int V> struct alignas(16) Pack {
    T v[V];
};

// p[0 .. V - 1] -> out, elements at or beyond `n` as 0; one 16-byte access when `vec` and all V are there
template <typename T, int V> __device__ __forceinline__ void load_pack(const T *p, int n, bool vec, float (&out)[V])
{
    if (vec && n >= V) {
        const Pack<T, V> k = *reinterpret_cast<const Pack<T, V> *>(p);
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = to_acc(k.v[j]);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = j < n ? to_acc(p[j]) : 0.0f;
    }
}

template <typename T, int V> __device__ __forceinline__ void store_pack(T *p, int n, bool vec, const float (&in)[V])
{
    if (vec && n >= V) {
        Pack<T, V> k;
#pragma unroll
        for (int j = 0; j < V; ++j) from_acc(k.v[j], in[j]);
        *reinterpret_cast<Pack<T, V> *>(p) = k;
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (j < n) from_acc(p[j], in[j]);
    }
}

// ---- statistics ------------------------------------------------------------------------------------------------------------
// Workgroup b owns chunk k of group (n, l, g): its mean and M2 by two sweeps over the registers.  The only chunk of a group
// writes mean and rstd; otherwise the pair goes to ws[2 b] for stat_combine_kernel.
template <typename TX>
__global__ __launch_bounds__(kThreads) void stat_kernel(const Levels xs, float *__restrict__ mean_out, float *__restrict__ rstd_out,
                                                        float *__restrict__ ws, const Geo geo, const float eps, const unsigned vecmask)
{
    constexpr int V = 16 / (int)sizeof(TX), R = kStatChunk / (kThreads * V);
    __shared__ float red[kWaves];
    const long long b = blockIdx.x;
    const int l = level_of(geo.sblock0, geo.L, b);
    const long long r = b - geo.sblock0[l];
    const int chunks = geo.schunks[l];
    const long long ng = r / chunks;
    const int k = (int)(r - ng * chunks);
    const long long n = ng / geo.G;
    const int g = (int)(ng - n * geo.G);
    const int M = geo.cpg * geo.HW[l];
    const int e0 = k * kStatChunk;
    const int cnt = min(kStatChunk, M - e0);
    const TX *base = (const TX *)xs.p[l] + (n * geo.C + (long long)g * geo.cpg) * geo.HW[l] + e0;
    const bool vec = (vecmask >> l) & 1u;
    float v[R][V];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int e = (i * kThreads + (int)threadIdx.x) * V;
        load_pack<TX, V>(base + e, cnt - e, vec, v[i]);
#pragma unroll
        for (int j = 0; j < V; ++j) s += v[i][j];
    }
    const float m = block_sum<kWaves>(s, red) / (float)cnt;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int e = (i * kThreads + (int)threadIdx.x) * V;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float d = e + j < cnt ? v[i][j] - m : 0.0f;
            q += d * d;
        }
    }
    const float M2 = block_sum<kWaves>(q, red);
    if (threadIdx.x == 0) {
        if (chunks == 1) {
            const long long o = (n * geo.L + l) * geo.G + g;
            mean_out[o] = m;
            rstd_out[o] = rsqrt_of(M2 / (float)M + eps);
        } else {
            ws[2 * b] = m;
            ws[2 * b + 1] = M2;
        }
    }
}

// one thread per group of several chunks: the chunks ascending, by Chan's formula
__global__ __launch_bounds__(kThreads) void stat_combine_kernel(const float *__restrict__ ws, float *__restrict__ mean_out,
                                                                float *__restrict__ rstd_out, const Geo geo, const float eps)
{
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (long long)geo.N * geo.L * geo.G) return;
    const int g = (int)(idx % geo.G), l = (int)((idx / geo.G) % geo.L);
    const long long n = idx / ((long long)geo.G * geo.L);
    const int chunks = geo.schunks[l];
    if (chunks == 1) return;
    const int M = geo.cpg * geo.HW[l];
    const float *part = ws + 2 * (geo.sblock0[l] + (n * geo.G + g) * chunks);
    float nA = (float)kStatChunk, mA = part[0], M2A = part[1];
    for (int k = 1; k < chunks; ++k) {
        const float nB = (float)min(kStatChunk, M - k * kStatChunk), mB = part[2 * k], M2B = part[2 * k + 1];
        const float d = mB - mA, nAB = nA + nB, f = nB / nAB;
        mA += d * f;
        M2A += M2B + (d * d) * (nA * f);
        nA = nAB;
    }
    mean_out[idx] = mA;
    rstd_out[idx] = rsqrt_of(M2A / (float)M + eps);
}

// ---- the tile ----------------------------------------------------------------------------------------------------------------
// The token side of a tile for V channels per thread: the 32 lanes of half a wave hold 32 / V channel vectors x V pixels (banks
// V q + pixel: all different), the two halves of a wave neighbouring channel ranges; a wave covers V pixels x 64 channels, the
// four waves 4 V pixels per pass.
template <int V> struct TokenSide {
    static constexpr int kQuads = 32 / V;
    static constexpr int kPassPixels = kWaves * V;
    static constexpr int kPasses = kTileP / kPassPixels;
    int q, po;
    __device__ __forceinline__ TokenSide()
    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        q = (lane & (kQuads - 1)) + kQuads * (lane >> 5);
        po = wave * V + (lane & 31) / kQuads;
    }
};

// Where a workgroup of the apply / grad_x launches works
struct TilePlace {
    int l, HW, p0, c0, npix;
    long long n;
    __device__ __forceinline__ TilePlace(const Geo &geo)
    {
        const long long b = blockIdx.x;
        l = level_of(geo.tblock0, geo.L, b);
        const long long r = b - geo.tblock0[l];
        n = r / geo.ptiles[l];
        p0 = (int)(r - n * geo.ptiles[l]) * kTileP;
        HW = geo.HW[l];
        c0 = blockIdx.y * kTileC;
        npix = min(kTileP, HW - p0);
    }
};

// grad_tokens of the tile's pixels [p0, p0 + npix) and channels [c0, c0 + 64) -> tile[channel][pixel]; 0 outside
template <typename TY>
__device__ __forceinline__ void load_token_tile(const TY *__restrict__ tok, const Geo &geo, long long n, int l, int p0, int npix, int c0,
                                                bool vecy, float *tile)
{
    constexpr int V = 16 / (int)sizeof(TY);
    const TokenSide<V> ts;
    const int c = c0 + ts.q * V;
#pragma unroll
    for (int pass = 0; pass < TokenSide<V>::kPasses; ++pass) {
        const int pl = pass * TokenSide<V>::kPassPixels + ts.po;
        float v[V];
        if (pl < npix) {
            load_pack<TY, V>(tok + ((n * geo.S + geo.start[l] + p0 + pl) * geo.C + c), geo.C - c, vecy, v);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = 0.0f;
        }
#pragma unroll
        for (int j = 0; j < V; ++j) tile[(ts.q * V + j) * kPitch + pl] = v[j];
    }
}

// ---- apply -------------------------------------------------------------------------------------------------------------------
template <typename TX, typename TP, typename TY>
__global__ __launch_bounds__(kThreads) void apply_kernel(const Levels xs, const Levels ws_, const Levels bs, const float *__restrict__ mean,
                                                         const float *__restrict__ rstd, TY *__restrict__ tokens, const Geo geo,
                                                         const int vecy_)
{
    constexpr int V = 16 / (int)sizeof(TY);
    __shared__ float tile[kTileC * kPitch];
    __shared__ float sm[kTileC], sr[kTileC], sw[kTileC], sb[kTileC];
    const TilePlace at(geo);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < kTileC) {
        const int c = at.c0 + (int)threadIdx.x;
        if (c < geo.C) {
            const long long o = (at.n * geo.L + at.l) * geo.G + c / geo.cpg;
            sm[threadIdx.x] = mean[o];
            sr[threadIdx.x] = rstd[o];
            sw[threadIdx.x] = to_acc(((const TP *)ws_.p[at.l])[c]);
            sb[threadIdx.x] = to_acc(((const TP *)bs.p[at.l])[c]);
        }
    }
    __syncthreads();
    const TX *x = (const TX *)xs.p[at.l] + (at.n * geo.C + at.c0) * at.HW + at.p0;
    if (lane < at.npix) {
#pragma unroll
        for (int i = 0; i < kRows; ++i) {
            const int cr = i * kWaves + wave;
            if (at.c0 + cr < geo.C)
                tile[cr * kPitch + lane] = ((to_acc(x[(long long)cr * at.HW + lane]) - sm[cr]) * sr[cr]) * sw[cr] + sb[cr];
        }
    }
    __syncthreads();
    const TokenSide<V> ts;
    const int c = at.c0 + ts.q * V;
    if (c >= geo.C) return;
#pragma unroll
    for (int pass = 0; pass < TokenSide<V>::kPasses; ++pass) {
        const int pl = pass * TokenSide<V>::kPassPixels + ts.po;
        if (pl >= at.npix) continue;
        float v[V];
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = c + j < geo.C ? tile[(ts.q * V + j) * kPitch + pl] : 0.0f;
        store_pack<TY, V>(tokens + ((at.n * geo.S + geo.start[at.l] + at.p0 + pl) * geo.C + c), geo.C - c, vecy_ != 0, v);
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------
// Workgroup (b, ctile) owns pixel chunk k of frame n of level l and 64 channels: sum_p(g) and sum_p(g * xhat) of the chunk
// -> ws[(b * C + c) * 2 + {0, 1}].
template <typename TX, typename TY>
__global__ __launch_bounds__(kThreads) void sums_kernel(const Levels xs, const float *__restrict__ mean, const float *__restrict__ rstd,
                                                        const TY *__restrict__ grad_tokens, float *__restrict__ ws, const Geo geo,
                                                        const unsigned wanted, const int vecy_)
{
    __shared__ float tile[kTileC * kPitch];
    __shared__ float sm[kTileC], sr[kTileC];
    const long long b = blockIdx.x;
    const int l = level_of(geo.bblock0, geo.L, b);
    if (!((wanted >> l) & 1u)) return;
    const long long r = b - geo.bblock0[l];
    const long long n = r / geo.bchunks[l];
    const int k = (int)(r - n * geo.bchunks[l]);
    const int HW = geo.HW[l], c0 = blockIdx.y * kTileC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < kTileC) {
        const int c = c0 + (int)threadIdx.x;
        if (c < geo.C) {
            const long long o = (n * geo.L + l) * geo.G + c / geo.cpg;
            sm[threadIdx.x] = mean[o];
            sr[threadIdx.x] = rstd[o];
        }
    }
    const TX *x = (const TX *)xs.p[l] + (n * geo.C + c0) * HW;
    float accA[kRows], accB[kRows];
#pragma unroll
    for (int i = 0; i < kRows; ++i) accA[i] = accB[i] = 0.0f;
    const int pend = min(HW, (k + 1) * kSumChunk);
    for (int p0 = k * kSumChunk; p0 < pend; p0 += kTileP) {
        __syncthreads();                                    // (sm / sr are there; the last tile is read)
        const int npix = min(kTileP, HW - p0);
        load_token_tile<TY>(grad_tokens, geo, n, l, p0, npix, c0, vecy_ != 0, tile);
        __syncthreads();
        if (lane < npix) {
#pragma unroll
            for (int i = 0; i < kRows; ++i) {
                const int cr = i * kWaves + wave;
                if (c0 + cr < geo.C) {
                    const float g = tile[cr * kPitch + lane];
                    const float xhat = (to_acc(x[(long long)cr * HW + p0 + lane]) - sm[cr]) * sr[cr];
                    accA[i] += g;
                    accB[i] += g * xhat;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
        const float a = wave_sum(accA[i]), bb = wave_sum(accB[i]);
        const int c = c0 + i * kWaves + wave;
        if (lane == 0 && c < geo.C) {
            ws[(b * geo.C + c) * 2] = a;
            ws[(b * geo.C + c) * 2 + 1] = bb;
        }
    }
}

// the chunks of (n, l, c), ascending
__device__ __forceinline__ void chunk_sums(const float *__restrict__ ws, const Geo &geo, long long n, int l, int c, float *a, float *bb)
{
    const float *part = ws + ((geo.bblock0[l] + n * geo.bchunks[l]) * geo.C + c) * 2;
    float sa = part[0], sb = part[1];
    for (int k = 1; k < geo.bchunks[l]; ++k) {
        sa += part[(long long)k * geo.C * 2];
        sb += part[(long long)k * geo.C * 2 + 1];
    }
    *a = sa;
    *bb = sb;
}

// Threads [0, L * C): grad_weight_l[c] and grad_bias_l[c], the frames ascending.  Threads [L * C, L * C + N * L * G): the two
// group terms c1 and c2 of (n, l, g) -> gterm, the channels ascending.
template <typename TP>
__global__ __launch_bounds__(kThreads) void sums_combine_kernel(const float *__restrict__ ws, const Levels weights, const OutLevels grad_w,
                                                                const OutLevels grad_b, float *__restrict__ gterm, const Geo geo,
                                                                const unsigned want_x)
{
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long params = (long long)geo.L * geo.C;
    if (idx < params) {
        const int l = (int)(idx / geo.C), c = (int)(idx - (long long)l * geo.C);
        TP *gw = (TP *)grad_w.p[l], *gb = (TP *)grad_b.p[l];
        if (!gw && !gb) return;
        float sa = 0.0f, sb = 0.0f;
        for (long long n = 0; n < geo.N; ++n) {
            float a, bb;
            chunk_sums(ws, geo, n, l, c, &a, &bb);
            sa = n == 0 ? a : sa + a;
            sb = n == 0 ? bb : sb + bb;
        }
        if (gw) from_acc(gw[c], sb);
        if (gb) from_acc(gb[c], sa);
        return;
    }
    const long long j = idx - params;
    if (j >= (long long)geo.N * geo.L * geo.G) return;
    const int g = (int)(j % geo.G), l = (int)((j / geo.G) % geo.L);
    if (!((want_x >> l) & 1u)) return;
    const long long n = j / ((long long)geo.G * geo.L);
    const TP *w = (const TP *)weights.p[l];
    float s1 = 0.0f, s2 = 0.0f;
    for (int c = g * geo.cpg; c < (g + 1) * geo.cpg; ++c) {
        float a, bb;
        chunk_sums(ws, geo, n, l, c, &a, &bb);
        const float wc = to_acc(w[c]);
        s1 += wc * a;
        s2 += wc * bb;
    }
    const float M = (float)(geo.cpg * geo.HW[l]);
    gterm[2 * j] = s1 / M;
    gterm[2 * j + 1] = s2 / M;
}

template <typename TX, typename TP, typename TY>
__global__ __launch_bounds__(kThreads) void grad_x_kernel(const Levels xs, const Levels weights, const float *__restrict__ mean,
                                                          const float *__restrict__ rstd, const float *__restrict__ gterm,
                                                          const TY *__restrict__ grad_tokens, const OutLevels grad_x, const Geo geo,
                                                          const int vecy_)
{
    __shared__ float tile[kTileC * kPitch];
    __shared__ float sm[kTileC], sr[kTileC], sw[kTileC], s1[kTileC], s2[kTileC];
    const TilePlace at(geo);
    TX *gx = (TX *)grad_x.p[at.l];
    if (!gx) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < kTileC) {
        const int c = at.c0 + (int)threadIdx.x;
        if (c < geo.C) {
            const long long o = (at.n * geo.L + at.l) * geo.G + c / geo.cpg;
            sm[threadIdx.x] = mean[o];
            sr[threadIdx.x] = rstd[o];
            sw[threadIdx.x] = to_acc(((const TP *)weights.p[at.l])[c]);
            s1[threadIdx.x] = gterm[2 * o];
            s2[threadIdx.x] = gterm[2 * o + 1];
        }
    }
    load_token_tile<TY>(grad_tokens, geo, at.n, at.l, at.p0, at.npix, at.c0, vecy_ != 0, tile);
    __syncthreads();
    if (lane >= at.npix) return;
    const long long off = (at.n * geo.C + at.c0) * at.HW + at.p0 + lane;
    const TX *x = (const TX *)xs.p[at.l] + off;
    gx += off;
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
        const int cr = i * kWaves + wave;
        if (at.c0 + cr < geo.C) {
            const float g = tile[cr * kPitch + lane];
            const float xhat = (to_acc(x[(long long)cr * at.HW]) - sm[cr]) * sr[cr];
            from_acc(gx[(long long)cr * at.HW], ((g * sw[cr] - s1[cr]) - xhat * s2[cr]) * sr[cr]);
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
int check_types(const inputproj_types *t)
{
    if (!t) return err.fail("null pointer: types");
    const bool known = elem_size(t->x) && elem_size(t->param) && elem_size(t->y) && t->x != kF64 && t->param != kF64 && t->y != kF64;
    const bool ok = known && (t->x == kF32 ? t->param == kF32 : (t->param == t->x || t->param == kF32) && (t->y == t->x || t->y == kF32));
    if (!ok)
        return err.fail("unsupported dtypes: float32 x takes float32 parameters and any y; 16-bit x takes parameters and y in its "
                        "own dtype or float32");
    return kOk;
}

int geo_of(const inputproj_shape *s, Geo *geo)
{
    if (!s) return err.fail("null pointer: shape");
    if (s->L < 1 || s->L > kMaxL) return err.fail("L must be in [1, %lld], got %lld", kMaxL, s->L);
    if (s->C < 1 || s->C > kMaxC) return err.fail("C must be in [1, %lld], got %lld", kMaxC, s->C);
    if (s->G < 1 || s->C % s->G) return err.fail("C = %lld must be a multiple of G = %lld >= 1", s->C, s->G);
    if (s->N < 0) return err.fail("N must not be negative, got %lld", s->N);
    *geo = Geo();
    geo->N = (int)s->N;
    geo->C = s->C;
    geo->G = s->G;
    geo->L = s->L;
    geo->cpg = s->C / s->G;
    long long S = 0;
    for (int l = 0; l < s->L; ++l) {
        if (s->H[l] < 0 || s->W[l] < 0) return err.fail("H and W must not be negative, got %lld x %lld", s->H[l], s->W[l]);
        const long long HW = (long long)s->H[l] * s->W[l];
        if (HW * geo->cpg > 0x7fffffffLL) return err.fail("a group of level %lld has %lld elements: more than 31 bits", l, HW * geo->cpg);
        geo->HW[l] = (int)HW;
        geo->start[l] = S;
        S += HW;
        geo->ptiles[l] = (int)cdiv(HW, kTileP);
        geo->schunks[l] = (int)cdiv(HW * geo->cpg, kStatChunk);
        geo->bchunks[l] = (int)cdiv(HW, kSumChunk);
        geo->tblock0[l + 1] = geo->tblock0[l] + s->N * geo->ptiles[l];
        geo->sblock0[l + 1] = geo->sblock0[l] + s->N * geo->G * geo->schunks[l];
        geo->bblock0[l + 1] = geo->bblock0[l] + s->N * geo->bchunks[l];
    }
    geo->S = S;
    if (s->N * S > 0x7fffffffLL) return err.fail("N * S = %lld tokens: more than 31 bits", s->N * S);
    return kOk;
}

template <typename H, typename F> int dispatch16(const inputproj_types &t, F &&f)
{
    if (t.param == kF32) return t.y == kF32 ? f(Tag<H>(), Tag<float>(), Tag<float>()) : f(Tag<H>(), Tag<float>(), Tag<H>());
    return t.y == kF32 ? f(Tag<H>(), Tag<H>(), Tag<float>()) : f(Tag<H>(), Tag<H>(), Tag<H>());
}

template <typename F> int dispatch_types(const inputproj_types &t, F &&f)
{
    if (t.x == kBF16) return dispatch16<__hip_bfloat16>(t, f);
    if (t.x == kF16) return dispatch16<__half>(t, f);
    if (t.y == kBF16) return f(Tag<float>(), Tag<float>(), Tag<__hip_bfloat16>());
    if (t.y == kF16) return f(Tag<float>(), Tag<float>(), Tag<__half>());
    return f(Tag<float>(), Tag<float>(), Tag<float>());
}

long long round256(long long bytes) { return (bytes + 255) / 256 * 256; }

bool several_chunks(const Geo &geo)
{
    for (int l = 0; l < geo.L; ++l)
        if (geo.schunks[l] > 1) return true;
    return false;
}

Levels levels_of(const inputproj_levels *t, int L)
{
    Levels out = {};
    for (int l = 0; t && l < L; ++l) out.p[l] = t->p[l];
    return out;
}

OutLevels out_levels_of(const inputproj_levels *t, int L)
{
    OutLevels out = {};
    for (int l = 0; t && l < L; ++l) out.p[l] = t->p[l];
    return out;
}

}  // namespace inputproj

using namespace inputproj;

extern "C" {

int inputproj_version(void) { return INPUTPROJ_ABI_VERSION; }

const char *inputproj_last_error(void) { return err.msg; }

int inputproj_tile(int which)
{
    switch (which) {
    case INPUTPROJ_TILE_PIXELS: return kTileP;
    case INPUTPROJ_TILE_CHANNELS: return kTileC;
    case INPUTPROJ_TILE_STAT_CHUNK: return kStatChunk;
    case INPUTPROJ_TILE_SUM_CHUNK: return kSumChunk;
    case INPUTPROJ_TILE_MAX_LEVELS: return kMaxL;
    case INPUTPROJ_TILE_MAX_CHANNELS: return kMaxC;
    default: return -1;
    }
}

long long inputproj_tokens(const inputproj_shape *shape)
{
    err.clear();
    Geo geo;
    if (geo_of(shape, &geo) != INPUTPROJ_OK) return INPUTPROJ_ERR_ARGUMENT;
    return geo.S;
}

long long inputproj_forward_workspace_bytes(const inputproj_shape *shape)
{
    err.clear();
    Geo geo;
    if (geo_of(shape, &geo) != INPUTPROJ_OK) return INPUTPROJ_ERR_ARGUMENT;
    return several_chunks(geo) ? round256(geo.sblock0[geo.L] * 2 * (long long)sizeof(float)) : 0;
}

long long inputproj_backward_workspace_bytes(const inputproj_shape *shape)
{
    err.clear();
    Geo geo;
    if (geo_of(shape, &geo) != INPUTPROJ_OK) return INPUTPROJ_ERR_ARGUMENT;
    return round256(geo.bblock0[geo.L] * geo.C * 2 * (long long)sizeof(float)) +
           round256((long long)geo.N * geo.L * geo.G * 2 * (long long)sizeof(float));
}

int inputproj_forward(const inputproj_types *types, const inputproj_levels *x, const inputproj_levels *weight,
                      const inputproj_levels *bias, double eps, const inputproj_shape *shape, void *workspace, void *tokens,
                      float *mean, float *rstd, void *stream)
{
    err.clear();
    Geo geo;
    if (geo_of(shape, &geo) != INPUTPROJ_OK || check_types(types) != INPUTPROJ_OK) return INPUTPROJ_ERR_ARGUMENT;
    if (!(eps == eps)) return err.fail("eps must be a number");
    if (!x || !weight || !bias) return err.fail("null pointer: the tables of x, weight and bias are required");
    if (geo.N == 0 || geo.S == 0) return INPUTPROJ_OK;
    if (!tokens || !mean || !rstd) return err.fail("null pointer: tokens, mean and rstd are required");
    const int xsize = elem_size(types->x);
    unsigned vecmask = 0;
    for (int l = 0; l < geo.L; ++l) {
        if (geo.HW[l] == 0) continue;
        if (!x->p[l] || !weight->p[l] || !bias->p[l]) return err.fail("null pointer: x, weight and bias of level %lld are required", l);
        if (aligned16(x->p[l]) && ((long long)geo.cpg * geo.HW[l] * xsize) % 16 == 0) vecmask |= 1u << l;
    }
    const bool combine = several_chunks(geo);
    if (combine && !workspace) return err.fail("null pointer: workspace is required when a group spans several chunks");
    if (!aligned16(workspace)) return err.fail("the workspace must be 16-byte aligned");
    const int vecy = geo.C % (16 / elem_size(types->y)) == 0 && aligned16(tokens);
    unsigned sgrid, tgrid, cgrid;
    if (err.grid_of(geo.sblock0[geo.L], &sgrid) != INPUTPROJ_OK || err.grid_of(geo.tblock0[geo.L], &tgrid) != INPUTPROJ_OK ||
        err.grid_of(cdiv((long long)geo.N * geo.L * geo.G, kThreads), &cgrid) != INPUTPROJ_OK)
        return INPUTPROJ_ERR_ARGUMENT;
    const Levels xs = levels_of(x, geo.L), wts = levels_of(weight, geo.L), bs = levels_of(bias, geo.L);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_types(*types, [&](auto tx, auto tp, auto ty) {
        typedef type_of<decltype(tx)> TX;
        typedef type_of<decltype(tp)> TP;
        typedef type_of<decltype(ty)> TY;
        hipLaunchKernelGGL((stat_kernel<TX>), dim3(sgrid), dim3(kThreads), 0, st, xs, mean, rstd, (float *)workspace, geo, (float)eps,
                           vecmask);
        if (combine)
            hipLaunchKernelGGL(stat_combine_kernel, dim3(cgrid), dim3(kThreads), 0, st, (const float *)workspace, mean, rstd, geo,
                               (float)eps);
        hipLaunchKernelGGL((apply_kernel<TX, TP, TY>), dim3(tgrid, (unsigned)cdiv(geo.C, kTileC)), dim3(kThreads), 0, st, xs, wts, bs,
                           (const float *)mean, (const float *)rstd, (TY *)tokens, geo, vecy);
        return err.check_launch("inputproj_forward");
    });
}

int inputproj_backward(const inputproj_types *types, const inputproj_levels *x, const inputproj_levels *weight, const float *mean,
                       const float *rstd, const void *grad_tokens, const inputproj_shape *shape, void *workspace,
                       const inputproj_levels *grad_x, const inputproj_levels *grad_weight, const inputproj_levels *grad_bias,
                       void *stream)
{
    err.clear();
    Geo geo;
    if (geo_of(shape, &geo) != INPUTPROJ_OK || check_types(types) != INPUTPROJ_OK) return INPUTPROJ_ERR_ARGUMENT;
    const OutLevels gx = out_levels_of(grad_x, geo.L), gw = out_levels_of(grad_weight, geo.L), gb = out_levels_of(grad_bias, geo.L);
    unsigned wanted = 0, want_x = 0;
    for (int l = 0; l < geo.L; ++l) {
        if (gx.p[l]) want_x |= 1u << l;
        if (gx.p[l] || gw.p[l] || gb.p[l]) wanted |= 1u << l;
    }
    if (!wanted) return err.fail("no gradient is asked for");
    if (geo.N == 0 || geo.S == 0) return err.fail("no elements: the gradients are zero and this call writes nothing");
    if (!x || !mean || !rstd || !grad_tokens) return err.fail("null pointer: x, mean, rstd and grad_tokens are required");
    for (int l = 0; l < geo.L; ++l) {
        if (!((wanted >> l) & 1u)) continue;
        if (geo.HW[l] == 0) return err.fail("level %lld has no pixels: its gradients are zero and this call writes nothing", l);
        if (!x->p[l]) return err.fail("null pointer: x of level %lld is required", l);
        if (gx.p[l] && !(weight && weight->p[l])) return err.fail("null pointer: weight of level %lld is required for its grad_x", l);
    }
    if (!workspace) return err.fail("null pointer: workspace is required");
    if (!aligned16(workspace)) return err.fail("the workspace must be 16-byte aligned");
    const int vecy = geo.C % (16 / elem_size(types->y)) == 0 && aligned16(grad_tokens);
    const unsigned ctiles = (unsigned)cdiv(geo.C, kTileC);
    unsigned bgrid, tgrid, cgrid;
    if (err.grid_of(geo.bblock0[geo.L], &bgrid) != INPUTPROJ_OK || err.grid_of(geo.tblock0[geo.L], &tgrid) != INPUTPROJ_OK ||
        err.grid_of(cdiv((long long)geo.L * geo.C + (long long)geo.N * geo.L * geo.G, kThreads), &cgrid) != INPUTPROJ_OK)
        return INPUTPROJ_ERR_ARGUMENT;
    float *ws = (float *)workspace;
    float *gterm = (float *)((char *)workspace + round256(geo.bblock0[geo.L] * geo.C * 2 * (long long)sizeof(float)));
    const Levels xs = levels_of(x, geo.L), wts = levels_of(weight, geo.L);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_types(*types, [&](auto tx, auto tp, auto ty) {
        typedef type_of<decltype(tx)> TX;
        typedef type_of<decltype(tp)> TP;
        typedef type_of<decltype(ty)> TY;
        hipLaunchKernelGGL((sums_kernel<TX, TY>), dim3(bgrid, ctiles), dim3(kThreads), 0, st, xs, mean, rstd, (const TY *)grad_tokens, ws,
                           geo, wanted, vecy);
        hipLaunchKernelGGL((sums_combine_kernel<TP>), dim3(cgrid), dim3(kThreads), 0, st, (const float *)ws, wts, gw, gb, gterm, geo,
                           want_x);
        if (want_x)
            hipLaunchKernelGGL((grad_x_kernel<TX, TP, TY>), dim3(tgrid, ctiles), dim3(kThreads), 0, st, xs, wts, mean, rstd,
                               (const float *)gterm, (const TY *)grad_tokens, gx, geo, vecy);
        return err.check_launch("inputproj_backward");
    });
}

}  // extern "C"
