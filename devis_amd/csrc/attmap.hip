// attmap.hip -- the mask head's attention maps (include/attmap.h): softmax over all heads and pixels
// of scale * q . k, fused so that the logits never exist in memory, and the softmax-gradient pass of its backward.
// gfx950, wave64, plain HIP, fp32 FMAs (fp64 for doubles); no atomics: every sum has a fixed order.
//
// Work decomposition of the forward: a workgroup owns (image b, head h, a tile of 256 * PPL pixels, a tile of kTQ queries).
// Lanes map to pixels -- k [B, n*c, H, W] is pixel-major per channel, so every load of k is a coalesced row segment -- and
// each lane keeps kTQ x PPL logits in registers, so a value of k is used kTQ times.  The (pre-scaled) queries of the tile sit
// in LDS and are read as broadcasts.  Query tiles are the fastest grid dimension: the workgroups that read one tile of k run
// together and share it through the caches.
#include "op_common.h"
#include "attmap.h"

namespace attmap {

using namespace devis;

static_assert(ATTMAP_OK == kOk && ATTMAP_ERR_ARGUMENT == kErrArgument && ATTMAP_ERR_HIP == kErrHip, "status codes");
static_assert(ATTMAP_F32 == kF32 && ATTMAP_F64 == kF64 && ATTMAP_BF16 == kBF16 && ATTMAP_F16 == kF16, "dtype codes");

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTQ = 8;              // queries per workgroup (a multiple of kWaves)
constexpr int kMaxC = 512;          // kTQ * c arithmetic values of LDS: 32 KiB for doubles at the bound

thread_local Status err;     // attmap_last_error()

// ---- forward -----------------------------------------------------------------------------------------------------------
// WRITE = false: pass 1, the tile's (maximum, sum of exp) per query -> ws[((row * n + h) * tiles + tile) * 2 + {0, 1}].
// WRITE = true:  pass 2, a row's n * tiles partials combined (a lane-strided loop and a butterfly: the same order in every
//                workgroup of the row, so they all hold the same bits), the logits recomputed, out written.
// Dynamic LDS: sq [c][kTQ], red [kTQ][kWaves], row [kTQ][2], all of the arithmetic type.
template <typename T, typename TO, int PPL, bool WRITE>
__global__ __launch_bounds__(kThreads) void attmap_fwd_kernel(const T *__restrict__ q, const T *__restrict__ k,
                                                              const unsigned char *__restrict__ mask,
                                                              typename Acc<T>::type *__restrict__ ws, TO *__restrict__ out,
                                                              const attmap_shape s, const typename Acc<T>::type scale,
                                                              const int tiles)
{
    typedef typename Acc<T>::type A;
    extern __shared__ __align__(16) unsigned char smem[];
    A *sq = reinterpret_cast<A *>(smem);
    A *red = sq + (size_t)s.c * kTQ;
    A *row = red + kTQ * kWaves;

    const int P = s.H * s.W, c = s.c;
    const int qtiles = (s.Q + kTQ - 1) / kTQ;
    const int qt = blockIdx.x % qtiles, tile = blockIdx.x / qtiles, h = blockIdx.y, b = blockIdx.z;
    const int q0 = qt * kTQ, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const A ninf = neg_inf(A());

    // a query past the end repeats the last one: computed, never stored
    for (int i = tid; i < c * kTQ; i += kThreads) {
        const int t = i % kTQ, cc = i / kTQ;
        const int qi = min(q0 + t, s.Q - 1);
        sq[i] = scale * (A)to_acc(q[(((long long)b * s.Q + qi) * s.n + h) * c + cc]);
    }
    __syncthreads();

    // a pixel past the end reads the last one (no bounds test in the loop) and counts as masked
    int at[PPL];
    bool dead[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        const int pix = tile * (kThreads * PPL) + j * kThreads + tid;
        at[j] = min(pix, P - 1);
        dead[j] = pix >= P || (mask && mask[(long long)b * P + at[j]] != 0);
    }
    A acc[kTQ][PPL];
#pragma unroll
    for (int t = 0; t < kTQ; ++t)
#pragma unroll
        for (int j = 0; j < PPL; ++j) acc[t][j] = (A)0;
    const T *kb = k + ((long long)b * s.n + h) * c * P;
#pragma unroll 4
    for (int cc = 0; cc < c; ++cc) {
        A kv[PPL];
#pragma unroll
        for (int j = 0; j < PPL; ++j) kv[j] = (A)to_acc(kb[(long long)cc * P + at[j]]);
#pragma unroll
        for (int t = 0; t < kTQ; ++t) {
            const A qv = sq[cc * kTQ + t];
#pragma unroll
            for (int j = 0; j < PPL; ++j) acc[t][j] = fma_of(qv, kv[j], acc[t][j]);
        }
    }
#pragma unroll
    for (int t = 0; t < kTQ; ++t)
#pragma unroll
        for (int j = 0; j < PPL; ++j)
            if (dead[j]) acc[t][j] = ninf;

    if (!WRITE) {
#pragma unroll
        for (int t = 0; t < kTQ; ++t) {
            A m = acc[t][0];
#pragma unroll
            for (int j = 1; j < PPL; ++j) m = max_of(m, acc[t][j]);
            m = wave_max(m);
            if (lane == 0) red[t * kWaves + wave] = m;
        }
        __syncthreads();
        A safe[kTQ];    // the tile's maximum; 0 for a tile with no live pixel, whose sum is then 0 (not NaN)
#pragma unroll
        for (int t = 0; t < kTQ; ++t) {
            A m = red[t * kWaves];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) m = max_of(m, red[t * kWaves + w]);
            safe[t] = m;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kTQ; ++t) {
            const A m = safe[t] == ninf ? (A)0 : safe[t];
            A sum = (A)0;
#pragma unroll
            for (int j = 0; j < PPL; ++j) sum += exp_of(acc[t][j] - m);
            sum = wave_sum(sum);
            if (lane == 0) red[t * kWaves + wave] = sum;
            if (tid == t) row[t * 2] = safe[t];
        }
        __syncthreads();
        if (tid < kTQ && q0 + tid < s.Q) {
            A sum = red[tid * kWaves];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) sum += red[tid * kWaves + w];
            A *dst = ws + (((((long long)b * s.Q + q0 + tid) * s.n + h) * tiles) + tile) * 2;
            dst[0] = row[tid * 2];
            dst[1] = sum;
        }
        return;
    }

    const int parts = s.n * tiles;
    for (int t = wave; t < kTQ; t += kWaves) {
        const int qi = min(q0 + t, s.Q - 1);
        const A *wp = ws + ((long long)b * s.Q + qi) * parts * 2;
        A m = ninf;
        for (int i = lane; i < parts; i += 64) m = max_of(m, wp[2 * i]);
        m = wave_max(m);
        const A safe = m == ninf ? (A)0 : m;
        A sum = (A)0;
        for (int i = lane; i < parts; i += 64) sum += wp[2 * i + 1] * exp_of(wp[2 * i] - safe);
        sum = wave_sum(sum);
        if (lane == 0) {
            row[t * 2] = m;                 // -inf for a fully masked row: exp(-inf - -inf) is the NaN the row is defined as
            row[t * 2 + 1] = (A)1 / sum;
        }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kTQ; ++t) {
        if (q0 + t >= s.Q) break;
        const A m = row[t * 2], inv = row[t * 2 + 1];
        TO *o = out + (((long long)b * s.Q + q0 + t) * s.n + h) * P;
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            const int pix = tile * (kThreads * PPL) + j * kThreads + tid;
            if (pix < P) from_acc(o[pix], exp_of(acc[t][j] - m) * inv);
        }
    }
}

// ---- backward: the softmax-gradient pass -------------------------------------------------------------------------------
// A workgroup owns (row, head, a tile of 256 * PPL pixels).
// WRITE = false: pass 1, sum of grad_out * out over the tile -> ws[(row * n + h) * tiles + tile].
// WRITE = true:  pass 2, r = the row's n * tiles partials in a fixed order (wave 0), then dl = scale * out * (grad_out - r).
template <typename T, typename TO, int PPL, bool WRITE>
__global__ __launch_bounds__(kThreads) void attmap_bwd_kernel(const TO *__restrict__ out, const TO *__restrict__ gout,
                                                              typename Acc<T>::type *__restrict__ ws, T *__restrict__ dl,
                                                              const attmap_shape s, const typename Acc<T>::type scale,
                                                              const int tiles)
{
    typedef typename Acc<T>::type A;
    __shared__ A red[kWaves];
    const int P = s.H * s.W;
    const int tile = blockIdx.x % tiles, h = (blockIdx.x / tiles) % s.n;
    const long long rowi = blockIdx.x / tiles / s.n;      // b * Q + q
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = (rowi * s.n + h) * P;
    A o[PPL], g[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        const int pix = tile * (kThreads * PPL) + j * kThreads + tid;
        const bool live = pix < P;
        o[j] = live ? (A)to_acc(out[base + pix]) : (A)0;
        g[j] = live ? (A)to_acc(gout[base + pix]) : (A)0;
    }
    if (!WRITE) {
        A sum = (A)0;
#pragma unroll
        for (int j = 0; j < PPL; ++j) sum = fma_of(g[j], o[j], sum);
        sum = wave_sum(sum);
        if (lane == 0) red[wave] = sum;
        __syncthreads();
        if (tid == 0) {
            A r = red[0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) r += red[w];
            ws[(rowi * s.n + h) * tiles + tile] = r;
        }
        return;
    }
    if (wave == 0) {
        const int parts = s.n * tiles;
        const A *wp = ws + rowi * parts;
        A sum = (A)0;
        for (int i = lane; i < parts; i += 64) sum += wp[i];
        sum = wave_sum(sum);
        if (lane == 0) red[0] = sum;
    }
    __syncthreads();
    const A r = red[0];
    const long long b = rowi / s.Q, qi = rowi % s.Q;
    T *d = dl + ((b * s.n + h) * s.Q + qi) * P;
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        const int pix = tile * (kThreads * PPL) + j * kThreads + tid;
        if (pix < P) from_acc(d[pix], scale * (o[j] * (g[j] - r)));
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------
// pixels per lane: large maps amortise a tile's reductions (and its reads of the queries) over four pixels a lane; small
// ones keep one, for more workgroups
int fwd_ppl(long long P) { return P >= 2048 ? 4 : 1; }
int bwd_ppl(long long P) { return P >= 2048 ? 8 : 1; }
int tiles_of(long long P, int ppl) { return (int)((P + (long long)kThreads * ppl - 1) / ((long long)kThreads * ppl)); }

int check_shape(const attmap_shape *s)
{
    if (!s) return err.fail("null pointer: shape");
    if (s->B < 0 || s->Q < 0 || s->n <= 0 || s->c <= 0 || s->H <= 0 || s->W <= 0)
        return err.fail("sizes must be positive (B and Q may be 0)");
    if (s->B > 65535 || s->n > 65535) return err.fail("B = %lld and n = %lld must not exceed 65535", s->B, s->n);
    if (s->c > kMaxC) return err.fail("c = %lld channels per head exceed the bound of %lld", s->c, kMaxC);
    if ((long long)s->H * s->W > 0x7fffffffLL) return err.fail("H * W = %lld does not fit 31 bits", (long long)s->H * s->W);
    return ATTMAP_OK;
}

int check_types(int dtype, int out_dtype)
{
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (out_dtype != dtype && !(out_dtype == ATTMAP_F32 && elem_size(dtype) == 2))
        return err.fail("out_dtype %lld must be dtype %lld itself, or ATTMAP_F32 beside a 16-bit dtype", out_dtype, dtype);
    return ATTMAP_OK;
}

template <typename T, typename TO>
int launch_forward(const void *q, const void *k, const unsigned char *mask, const attmap_shape &s, double scale, void *ws,
                   void *out, hipStream_t st)
{
    typedef typename Acc<T>::type A;
    const long long P = (long long)s.H * s.W;
    const int ppl = fwd_ppl(P), tiles = tiles_of(P, ppl);
    unsigned gx;
    if (err.grid_of((long long)((s.Q + kTQ - 1) / kTQ) * tiles, &gx)) return ATTMAP_ERR_ARGUMENT;
    const dim3 grid(gx, (unsigned)s.n, (unsigned)s.B), block(kThreads);
    const size_t lds = ((size_t)s.c * kTQ + kTQ * kWaves + kTQ * 2) * sizeof(A);
#define ATTMAP_FWD(PPL, WRITE)                                                                                          \
    hipLaunchKernelGGL((attmap_fwd_kernel<T, TO, PPL, WRITE>), grid, block, lds, st, (const T *)q, (const T *)k, mask,   \
                       (A *)ws, (TO *)out, s, (A)scale, tiles)
    if (ppl == 4) { ATTMAP_FWD(4, false); ATTMAP_FWD(4, true); }
    else { ATTMAP_FWD(1, false); ATTMAP_FWD(1, true); }
#undef ATTMAP_FWD
    return err.check_launch("attmap_fwd_kernel");
}

template <typename T, typename TO>
int launch_backward(const void *out, const void *gout, const attmap_shape &s, double scale, void *ws, void *dl, hipStream_t st)
{
    typedef typename Acc<T>::type A;
    const long long P = (long long)s.H * s.W;
    const int ppl = bwd_ppl(P), tiles = tiles_of(P, ppl);
    unsigned gx;
    if (err.grid_of((long long)s.B * s.Q * s.n * tiles, &gx)) return ATTMAP_ERR_ARGUMENT;
    const dim3 grid(gx), block(kThreads);
#define ATTMAP_BWD(PPL, WRITE)                                                                                          \
    hipLaunchKernelGGL((attmap_bwd_kernel<T, TO, PPL, WRITE>), grid, block, 0, st, (const TO *)out, (const TO *)gout,    \
                       (A *)ws, (T *)dl, s, (A)scale, tiles)
    if (ppl == 8) { ATTMAP_BWD(8, false); ATTMAP_BWD(8, true); }
    else { ATTMAP_BWD(1, false); ATTMAP_BWD(1, true); }
#undef ATTMAP_BWD
    return err.check_launch("attmap_bwd_kernel");
}

}  // namespace attmap

using namespace attmap;

extern "C" {

int attmap_version(void) { return ATTMAP_ABI_VERSION; }

const char *attmap_last_error(void) { return err.msg; }

long long attmap_workspace_bytes(int dtype, const attmap_shape *shape)
{
    err.clear();
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (check_shape(shape) != ATTMAP_OK) return ATTMAP_ERR_ARGUMENT;
    const long long P = (long long)shape->H * shape->W;
    // the forward's partials: the backward's tiles are no smaller and it keeps one value per tile
    const long long bytes = (long long)shape->B * shape->Q * shape->n * tiles_of(P, fwd_ppl(P)) * 2 * acc_size(dtype);
    return (bytes + 255) / 256 * 256;
}

int attmap_forward(int dtype, int out_dtype, const void *q, const void *k, const unsigned char *mask,
                   const attmap_shape *shape, double scale, void *workspace, void *out, void *stream)
{
    err.clear();
    if (check_types(dtype, out_dtype) != ATTMAP_OK || check_shape(shape) != ATTMAP_OK) return ATTMAP_ERR_ARGUMENT;
    if (shape->B == 0 || shape->Q == 0) return ATTMAP_OK;
    if (!q || !k || !workspace || !out) return err.fail("null pointer: q, k, workspace and out are required");
    hipStream_t st = (hipStream_t)stream;
    return dispatch(dtype, out_dtype != dtype, [&](auto t, auto to) {
        return launch_forward<type_of<decltype(t)>, type_of<decltype(to)>>(q, k, mask, *shape, scale, workspace, out, st);
    });
}

int attmap_backward(int grads, int dtype, int out_dtype, const void *out, const void *grad_out, const attmap_shape *shape,
                    double scale, void *workspace, void *dl, void *stream)
{
    err.clear();
    if (check_types(dtype, out_dtype) != ATTMAP_OK) return ATTMAP_ERR_ARGUMENT;
    if (grads < 0 || grads > (ATTMAP_GRAD_Q | ATTMAP_GRAD_K))
        return err.fail("grads = %lld is not a mask of ATTMAP_GRAD_Q and ATTMAP_GRAD_K", grads);
    if (check_shape(shape) != ATTMAP_OK) return ATTMAP_ERR_ARGUMENT;
    if (shape->B == 0 || shape->Q == 0 || grads == 0) return ATTMAP_OK;
    if (!out || !grad_out || !workspace || !dl) return err.fail("null pointer: out, grad_out, workspace and dl are required");
    hipStream_t st = (hipStream_t)stream;
    return dispatch(dtype, out_dtype != dtype, [&](auto t, auto to) {
        return launch_backward<type_of<decltype(t)>, type_of<decltype(to)>>(out, grad_out, *shape, scale, workspace, dl, st);
    });
}

}  // extern "C"
