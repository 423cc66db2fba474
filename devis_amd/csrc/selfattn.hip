// selfattn.hip -- the decoder's query self-attention between the projections of nn.MultiheadAttention (include/selfattn.h;
// DESIGN.md section 20): out = dropout(softmax(q k^T / sqrt(D))) v per batch entry and head, forward and backward.  gfx950,
// wave64, plain HIP.  One wave owns 16 rows and walks the other sequence in tiles of 16; the logit tile stays in the
// accumulator registers of v_mfma_f32_16x16x4_f32 and is the operand of the product that follows it.  There is no LDS, no
// atomic and nothing is zeroed.  The dropout mask is Philox4x32-10 of (seed, row, key / 4), recomputed by the backward, and
// the seed is read on the device.
#include "op_common.h"       // (fp contraction off)
#include "philox.h"
#include "selfattn.h"

namespace selfattn {

using namespace devis;

static_assert(SELFATTN_OK == kOk && SELFATTN_ERR_ARGUMENT == kErrArgument && SELFATTN_ERR_HIP == kErrHip, "status codes");
static_assert(SELFATTN_F32 == kF32 && SELFATTN_F64 == kF64 && SELFATTN_BF16 == kBF16 && SELFATTN_F16 == kF16, "dtype codes");

constexpr int kTile = 16;                       // rows of a wave, and rows of a tile of the other sequence
constexpr int kMaxD = SELFATTN_MAX_HEAD_DIM;

thread_local Status err;     // selfattn_last_error()

typedef float f32x4 __attribute__((ext_vector_type(4)));

// D[i][j] += sum over the 4 k-slots of A[i][slot] * B[slot][j]: lane l gives A[l & 15][l >> 4] and B[l >> 4][l & 15] and
// holds D[4 * (l >> 4) + reg][l & 15]
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0); }

struct Strides {
    long long seq, batch;                       // elements
};

// the problem, as the kernels take it
struct Problem {
    int L, S, H, D;
    float inv_sqrt_d;                           // 1 / sqrt(D)
    unsigned long long threshold;               // the mask (include/selfattn.h)
    float keep_scale;
    int vec;                                    // every pointer 16-byte aligned, every stride a multiple of 4 elements
};

// ---- loads and stores -------------------------------------------------------------------------------------------------------
template <typename T> struct alignas(sizeof(T) * 4) Quad {
    T v[4];
};

// p[0 .. n) -> out[0 .. n), out[n .. NQ) = 0; a row that is not `valid` is zeros and is not read.  `vec`: n % 4 == 0 and
// p is 8 / 16-byte aligned.
template <typename T, int NQ> __device__ __forceinline__ void load_chunk(const T *p, int n, bool valid, bool vec, float (&out)[NQ])
{
#pragma unroll
    for (int t = 0; t < NQ; ++t) out[t] = 0.0f;
    if (!valid) return;
    if (vec) {
#pragma unroll
        for (int t = 0; t < NQ; t += 4)
            if (t < n) {
                const Quad<T> q = *reinterpret_cast<const Quad<T> *>(p + t);
#pragma unroll
                for (int j = 0; j < 4; ++j) out[t + j] = to_acc(q.v[j]);
            }
    } else {
#pragma unroll
        for (int t = 0; t < NQ; ++t)
            if (t < n) out[t] = to_acc(p[t]);
    }
}

template <typename T> __device__ __forceinline__ float load_one(const T *p, bool valid) { return valid ? to_acc(*p) : 0.0f; }

// the registers of an accumulator tile, times `factor`, -> p[0 .. 3]
template <typename T> __device__ __forceinline__ void store_quad(T *p, bool vec, f32x4 acc, float factor)
{
    if (vec) {
        Quad<T> q;
#pragma unroll
        for (int j = 0; j < 4; ++j) from_acc(q.v[j], acc[j] * factor);
        *reinterpret_cast<Quad<T> *>(p) = q;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) from_acc(p[j], acc[j] * factor);
    }
}

// sum_t a[t] * b[t] over the channels of a head as a 16 x 16 tile: rows are a's rows, columns b's.  Lane (c, g) holds the
// channels g * n .. g * n + n - 1 of row c of each -- the summation index is permuted the same way in both.
template <int NQ> __device__ __forceinline__ f32x4 dot_tile(const float (&a)[NQ], const float (&b)[NQ], int n)
{
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < NQ; ++t)
        if (t < n) acc = mfma4(a[t], b[t], acc);
    return acc;
}

// the sum over the four lanes c, c + 16, c + 32, c + 48 in each of them
__device__ __forceinline__ float column_sum(float v)
{
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

__device__ __forceinline__ float column_max(float v)
{
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    v = fmaxf(v, __shfl_xor(v, 32, 64));
    return v;
}

// bit r: probability (row, 4 * quad + r) is kept
__device__ __forceinline__ unsigned keep_of(long long seed, long long row, unsigned quad, unsigned long long threshold)
{
    unsigned w[4];
    philox4x32_10((unsigned)seed, (unsigned)((unsigned long long)seed >> 32), (unsigned)row,
                  (unsigned)((unsigned long long)row >> 32), quad, 1u, w);
    unsigned keep = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) keep |= (unsigned long long)w[j] >= threshold ? 1u << j : 0u;
    return keep;
}

// delta = sum_d(dO * O) of the row whose chunk this lane holds, in each of its four lanes: t ascending, then the lanes
template <int NQ> __device__ __forceinline__ float delta_of(const float (&dof)[NQ], const float (&of)[NQ], int n)
{
    float s = 0.0f;
#pragma unroll
    for (int t = 0; t < NQ; ++t)
        if (t < n) s += dof[t] * of[t];
    return column_sum(s);
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
// Wave (blockIdx.x, blockIdx.y = n * H + h): the queries [16 * blockIdx.x, ...).  CT tiles of 16 channels cover a head.
template <typename T, int CT>
__global__ __launch_bounds__(64) void forward_kernel(const T *__restrict__ q, const Strides qs, const T *__restrict__ k,
                                                     const Strides ks, const T *__restrict__ v, const Strides vs,
                                                     const long long *__restrict__ seed, T *__restrict__ out,
                                                     float *__restrict__ lse, float *__restrict__ out_acc, const Problem pb,
                                                     const int N)
{
    constexpr int NQ = 4 * CT;
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const int nh = blockIdx.y, nb = nh / pb.H, h = nh - nb * pb.H;
    const int L = pb.L, S = pb.S, D = pb.D, n = D >> 2;
    const long long i = (long long)blockIdx.x * kTile + c;
    const bool chunk_vec = pb.vec && (n & 3) == 0;
    const long long head = (long long)h * D;
    const long long row = (long long)nh * L + i;
    const long long sd = seed ? *seed : 0;
    float qf[NQ];
    load_chunk<T, NQ>(q + i * qs.seq + nb * qs.batch + head + g * n, n, i < L, chunk_vec, qf);
    f32x4 o[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) o[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float m = -INFINITY, l = 0.0f;                  // of query c: the maximum so far, this lane's share of the sum
    // the operands of the tile at j0: this lane's chunk of key j0 + c, and channel ct * 16 + c of the keys j0 + 4 g + r
    auto load_tile = [&](long long j0, float (&kf)[NQ], float (&vt)[CT][4]) {
        load_chunk<T, NQ>(k + (j0 + c) * ks.seq + nb * ks.batch + head + g * n, n, j0 + c < S, chunk_vec, kf);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long j = j0 + 4 * g + r;
                vt[ct][r] = load_one(v + j * vs.seq + nb * vs.batch + head + ct * 16 + c, ct * 16 + c < D && j < S);
            }
    };
    float kf[NQ], vt[CT][4];
    load_tile(0, kf, vt);
    for (long long j0 = 0; j0 < S; j0 += kTile) {
        float k_next[NQ], v_next[CT][4];            // the next tile is in flight while this one is computed
        load_tile(j0 + kTile, k_next, v_next);
        const f32x4 st = dot_tile<NQ>(kf, qf, n);   // S^T: register r is key j0 + 4 g + r, the lane column query c
        float s[4], tile_max = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[r] = j0 + 4 * g + r < S ? st[r] * pb.inv_sqrt_d : -INFINITY;
            tile_max = fmaxf(tile_max, s[r]);
        }
        const float m_new = fmaxf(m, column_max(tile_max));
        const float alpha = expf(m - m_new);
        const unsigned keep = seed ? keep_of(sd, row, (unsigned)((j0 >> 2) + g), pb.threshold) : 0xfu;
        float pd[4], sum = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = expf(s[r] - m_new);
            sum += e;
            pd[r] = (keep >> r) & 1u ? e * pb.keep_scale : 0.0f;
        }
        l = l * alpha + sum;
        m = m_new;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            if (ct * 16 >= D) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[ct][r] *= alpha;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[ct] = mfma4(vt[ct][r], pd[r], o[ct]);       // O^T += V^T P^T: slot g is key j0 + 4 g + r
        }
#pragma unroll
        for (int t = 0; t < NQ; ++t) kf[t] = k_next[t];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) vt[ct][r] = v_next[ct][r];
    }
    const float total = column_sum(l);
    if (i >= L) return;
    if (lse && g == 0) lse[row] = m + logf(total);
    const float inv = 1.0f / total;
    const long long dense = ((long long)i * N + nb) * ((long long)pb.H * D) + head;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int d0 = ct * 16 + 4 * g;             // register r is channel d0 + r
        if (d0 >= D) continue;
        store_quad(out + dense + d0, pb.vec != 0, o[ct], inv);
        if (out_acc) store_quad(out_acc + dense + d0, pb.vec != 0, o[ct], inv);       // before the rounding to T: the backward's
    }
}

// ---- backward: grad_q ---------------------------------------------------------------------------------------------------------
// The forward's geometry.  P^T is recomputed from lse, dP^T = V dO^T lands in its layout, and dS^T is the B operand of
// dQ^T += K^T dS^T.
template <typename T, int CT>
__global__ __launch_bounds__(64) void backward_q_kernel(const T *__restrict__ q, const Strides qs, const T *__restrict__ k,
                                                        const Strides ks, const T *__restrict__ v, const Strides vs,
                                                        const float *__restrict__ out, const T *__restrict__ grad_out,
                                                        const float *__restrict__ lse, const long long *__restrict__ seed,
                                                        T *__restrict__ grad_q, const Problem pb, const int N)
{
    constexpr int NQ = 4 * CT;
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const int nh = blockIdx.y, nb = nh / pb.H, h = nh - nb * pb.H;
    const int L = pb.L, S = pb.S, D = pb.D, n = D >> 2;
    const long long i = (long long)blockIdx.x * kTile + c;
    const bool chunk_vec = pb.vec && (n & 3) == 0;
    const long long head = (long long)h * D;
    const long long row = (long long)nh * L + i;
    const long long sd = seed ? *seed : 0;
    const long long dense = ((long long)i * N + nb) * ((long long)pb.H * D) + head;        // of out, grad_out and grad_q
    float qf[NQ], dof[NQ], of[NQ];
    load_chunk<T, NQ>(q + i * qs.seq + nb * qs.batch + head + g * n, n, i < L, chunk_vec, qf);
    load_chunk<T, NQ>(grad_out + dense + g * n, n, i < L, chunk_vec, dof);
    load_chunk<float, NQ>(out + dense + g * n, n, i < L, chunk_vec, of);
    const float delta = delta_of<NQ>(dof, of, n);
    const float lse_i = i < L ? lse[row] : 0.0f;
    f32x4 dq[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) dq[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    // the operands of the tile at j0: this lane's chunks of key j0 + c, and channel ct * 16 + c of the keys j0 + 4 g + r
    auto load_tile = [&](long long j0, float (&kf)[NQ], float (&vf)[NQ], float (&kt)[CT][4]) {
        load_chunk<T, NQ>(k + (j0 + c) * ks.seq + nb * ks.batch + head + g * n, n, j0 + c < S, chunk_vec, kf);
        load_chunk<T, NQ>(v + (j0 + c) * vs.seq + nb * vs.batch + head + g * n, n, j0 + c < S, chunk_vec, vf);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long j = j0 + 4 * g + r;
                kt[ct][r] = load_one(k + j * ks.seq + nb * ks.batch + head + ct * 16 + c, ct * 16 + c < D && j < S);
            }
    };
    float kf[NQ], vf[NQ], kt[CT][4];
    load_tile(0, kf, vf, kt);
    for (long long j0 = 0; j0 < S; j0 += kTile) {
        float k_next[NQ], v_next[NQ], kt_next[CT][4];       // the next tile is in flight while this one is computed
        load_tile(j0 + kTile, k_next, v_next, kt_next);
        const f32x4 st = dot_tile<NQ>(kf, qf, n);
        const f32x4 dpt = dot_tile<NQ>(vf, dof, n);
        const unsigned keep = seed ? keep_of(sd, row, (unsigned)((j0 >> 2) + g), pb.threshold) : 0xfu;
        float ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float prob = j0 + 4 * g + r < S ? expf(st[r] * pb.inv_sqrt_d - lse_i) : 0.0f;
            const float dp = (keep >> r) & 1u ? dpt[r] * pb.keep_scale : 0.0f;
            ds[r] = prob * (dp - delta);
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            if (ct * 16 >= D) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) dq[ct] = mfma4(kt[ct][r], ds[r], dq[ct]);     // dQ^T += K^T dS^T
        }
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            kf[t] = k_next[t];
            vf[t] = v_next[t];
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) kt[ct][r] = kt_next[ct][r];
    }
    if (i >= L) return;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int d0 = ct * 16 + 4 * g;
        if (d0 < D) store_quad(grad_q + dense + d0, pb.vec != 0, dq[ct], pb.inv_sqrt_d);
    }
}

// ---- backward: grad_k and grad_v ----------------------------------------------------------------------------------------------
// Wave (blockIdx.x, n * H + h): the keys [16 * blockIdx.x, ...), walking the queries.  The tile is untransposed -- register r
// is query i0 + 4 g + r, the lane column key c --, so that it is the B operand of dV^T += dO^T P and dK^T += Q^T dS.
template <typename T, int CT>
__global__ __launch_bounds__(64) void backward_kv_kernel(const T *__restrict__ q, const Strides qs, const T *__restrict__ k,
                                                         const Strides ks, const T *__restrict__ v, const Strides vs,
                                                         const float *__restrict__ out, const T *__restrict__ grad_out,
                                                         const float *__restrict__ lse, const long long *__restrict__ seed,
                                                         T *__restrict__ grad_k, T *__restrict__ grad_v, const Problem pb,
                                                         const int N)
{
    constexpr int NQ = 4 * CT;
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const int nh = blockIdx.y, nb = nh / pb.H, h = nh - nb * pb.H;
    const int L = pb.L, S = pb.S, D = pb.D, n = D >> 2;
    const long long j = (long long)blockIdx.x * kTile + c;
    const bool chunk_vec = pb.vec && (n & 3) == 0;
    const long long head = (long long)h * D;
    const long long E = (long long)pb.H * D;
    const long long sd = seed ? *seed : 0;
    const bool want_k = grad_k != nullptr, want_v = grad_v != nullptr;
    float kf[NQ], vf[NQ];
    load_chunk<T, NQ>(k + (long long)j * ks.seq + nb * ks.batch + head + g * n, n, j < S, chunk_vec, kf);
    load_chunk<T, NQ>(v + (long long)j * vs.seq + nb * vs.batch + head + g * n, n, want_k && j < S, chunk_vec, vf);
    f32x4 dk[CT], dv[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) dk[ct] = dv[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (long long i0 = 0; i0 < L; i0 += kTile) {
        const long long ic = i0 + c;                     // the query whose chunks this lane loads
        const long long dense = ((long long)ic * N + nb) * E + head;
        float qf[NQ], dof[NQ];
        load_chunk<T, NQ>(q + (long long)ic * qs.seq + nb * qs.batch + head + g * n, n, ic < L, chunk_vec, qf);
        load_chunk<T, NQ>(grad_out + dense + g * n, n, want_k && ic < L, chunk_vec, dof);
        const f32x4 st = dot_tile<NQ>(qf, kf, n);
        float prob[4], pd[4];
        unsigned keep = 0xfu;                       // bit r: (query i0 + 4 g + r, key j)
        if (seed) {
            keep = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long row = (long long)nh * L + i0 + 4 * g + r;
                keep |= ((keep_of(sd, row, (unsigned)j >> 2, pb.threshold) >> (j & 3)) & 1u) << r;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long i = i0 + 4 * g + r;
            prob[r] = i < L && j < S ? expf(st[r] * pb.inv_sqrt_d - lse[(long long)nh * L + i]) : 0.0f;
            pd[r] = (keep >> r) & 1u ? prob[r] * pb.keep_scale : 0.0f;
        }
        if (want_v) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                if (ct * 16 >= D) continue;
                const bool channel = ct * 16 + c < D;
#pragma unroll
                for (int r = 0; r < 4; ++r) {       // dV^T += dO^T P: k-slot g of step r is query i0 + 4 g + r
                    const long long i = i0 + 4 * g + r;
                    const float a = load_one(grad_out + ((long long)i * N + nb) * E + head + ct * 16 + c, channel && i < L);
                    dv[ct] = mfma4(a, pd[r], dv[ct]);
                }
            }
        }
        if (want_k) {
            float of[NQ];
            load_chunk<float, NQ>(out + dense + g * n, n, ic < L, chunk_vec, of);
            const float delta_c = delta_of<NQ>(dof, of, n);             // of query i0 + c
            const f32x4 dpt = dot_tile<NQ>(dof, vf, n);
            float ds[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float delta = __shfl(delta_c, 4 * g + r, 64);     // of query i0 + 4 g + r
                const float dp = (keep >> r) & 1u ? dpt[r] * pb.keep_scale : 0.0f;
                ds[r] = prob[r] * (dp - delta);
            }
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                if (ct * 16 >= D) continue;
                const bool channel = ct * 16 + c < D;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long long i = i0 + 4 * g + r;
                    const float a = load_one(q + (long long)i * qs.seq + nb * qs.batch + head + ct * 16 + c, channel && i < L);
                    dk[ct] = mfma4(a, ds[r], dk[ct]);
                }
            }
        }
    }
    if (j >= S) return;
    const long long dst = ((long long)j * N + nb) * E + head;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int d0 = ct * 16 + 4 * g;
        if (d0 >= D) continue;
        if (want_k) store_quad(grad_k + dst + d0, pb.vec != 0, dk[ct], pb.inv_sqrt_d);
        if (want_v) store_quad(grad_v + dst + d0, pb.vec != 0, dv[ct], 1.0f);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
constexpr long long kMax31 = 0x7fffffffLL;

int check_shape(const selfattn_shape *s)
{
    if (!s) return err.fail("null pointer: shape");
    if (s->L < 0 || s->S < 0 || s->N < 0) return err.fail("L, S and N must not be negative");
    if (s->L > kMax31 || s->S > kMax31 || s->N > kMax31 || s->E > kMax31)
        return err.fail("L, S, N and E must fit 31 bits (L = %lld, S = %lld)", s->L, s->S);
    if (s->H < 1 || s->E < 1) return err.fail("E and the number of heads must be positive, got %lld and %lld", s->E, s->H);
    if (s->E % s->H) return err.fail("E = %lld is not divisible by %lld heads", s->E, s->H);
    const long long D = s->E / s->H;
    if (D % 4 || D < 4 || D > kMaxD)
        return err.fail("the head dimension must be a multiple of 4 in [4, %lld], got %lld", (long long)kMaxD, D);
    if (s->N * s->H > kMax31) return err.fail("N * H = %lld does not fit 31 bits", s->N * s->H);
    return SELFATTN_OK;
}

int check_view(const selfattn_view *view, const char *name)
{
    if (!view) return err.fail("null pointer: a view is required for q, k and v");
    if (view->channel != 1) {
        snprintf(err.msg, sizeof(err.msg), "the last stride of %s must be 1, got %lld", name, view->channel);
        return SELFATTN_ERR_ARGUMENT;
    }
    if (view->seq < 0 || view->batch < 0 || view->seq > kMax31 || view->batch > kMax31) {
        snprintf(err.msg, sizeof(err.msg), "the strides of %s must be in [0, 2^31) to fit 31 bits, got %lld and %lld", name,
                 view->seq, view->batch);
        return SELFATTN_ERR_ARGUMENT;
    }
    return SELFATTN_OK;
}

// p -> threshold and scale (include/selfattn.h)
int mask_of(double p, const long long *seed, unsigned long long *threshold, double *scale)
{
    if (!(p >= 0.0 && p <= 1.0)) return err.fail("p must be in [0, 1]");
    if (p > 0.0 && !seed) return err.fail("null pointer: seed is required when p > 0");
    *threshold = (unsigned long long)(p * 4294967296.0);        // (the product is exact or rounds down to below 2^32 + 1)
    *scale = p < 1.0 ? 1.0 / (1.0 - p) : 0.0;
    return SELFATTN_OK;
}

int check_dtype(int dtype)
{
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (dtype == kF64) return err.fail("unsupported dtype: float64 (float32, bfloat16 or float16)");
    return SELFATTN_OK;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }       // (NULL is aligned)

bool quads(const selfattn_view &v) { return v.seq % 4 == 0 && v.batch % 4 == 0; }

Problem problem_of(const selfattn_shape &s, unsigned long long threshold, double scale, bool vec)
{
    Problem pb;
    pb.L = (int)s.L;
    pb.S = (int)s.S;
    pb.H = (int)s.H;
    pb.D = (int)(s.E / s.H);
    pb.inv_sqrt_d = (float)(1.0 / sqrt((double)pb.D));
    pb.threshold = threshold;
    pb.keep_scale = (float)scale;
    pb.vec = vec ? 1 : 0;
    return pb;
}

Strides strides_of(const selfattn_view &v) { return Strides{v.seq, v.batch}; }

template <int N> struct Tiles { static constexpr int value = N; };

// f(Tag<T>, Tiles<CT>) for the storage type and the CT in 1 .. 4 tiles of 16 channels that cover D
template <typename F> int dispatch_kernel(int dtype, int D, F &&f)
{
    return dispatch(dtype, [&](auto t) {
        typedef type_of<decltype(t)> T;
        if constexpr (sizeof(T) == 8) {
            return err.fail("unsupported dtype: float64");
        } else {
            switch ((D + 15) / 16) {
            case 1: return f(Tag<T>(), Tiles<1>());
            case 2: return f(Tag<T>(), Tiles<2>());
            case 3: return f(Tag<T>(), Tiles<3>());
            default: return f(Tag<T>(), Tiles<4>());
            }
        }
    });
}

// the grid of `rows` rows per (n, h)
int grid_of(long long rows, const selfattn_shape &s, dim3 *grid)
{
    if (s.N * s.H > 65535) return err.fail("N * H = %lld is more than the 65535 a launch takes", s.N * s.H);
    unsigned x;
    if (err.grid_of(cdiv(rows, kTile), &x) != SELFATTN_OK) return SELFATTN_ERR_ARGUMENT;
    *grid = dim3(x, (unsigned)(s.N * s.H));
    return SELFATTN_OK;
}

}  // namespace selfattn

using namespace selfattn;

extern "C" {

int selfattn_version(void) { return SELFATTN_ABI_VERSION; }

const char *selfattn_last_error(void) { return err.msg; }

int selfattn_forward(int dtype, const void *q, const selfattn_view *q_view, const void *k, const selfattn_view *k_view,
                     const void *v, const selfattn_view *v_view, const long long *seed, double p, const selfattn_shape *shape,
                     void *out, void *lse, void *out_acc, void *stream)
{
    err.clear();
    if (check_dtype(dtype) != SELFATTN_OK || check_shape(shape) != SELFATTN_OK) return SELFATTN_ERR_ARGUMENT;
    unsigned long long threshold;
    double scale;
    if (mask_of(p, seed, &threshold, &scale) != SELFATTN_OK) return SELFATTN_ERR_ARGUMENT;
    const selfattn_shape &s = *shape;
    if (s.L == 0 || s.N == 0 || s.S == 0) return 0;
    if (check_view(q_view, "q") != SELFATTN_OK || check_view(k_view, "k") != SELFATTN_OK || check_view(v_view, "v") != SELFATTN_OK)
        return SELFATTN_ERR_ARGUMENT;
    if (!q || !k || !v || !out) return err.fail("null pointer: q, k, v and out are required");
    dim3 grid;
    if (grid_of(s.L, s, &grid) != SELFATTN_OK) return SELFATTN_ERR_ARGUMENT;
    const bool vec = aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(out_acc) && quads(*q_view) &&
                     quads(*k_view) && quads(*v_view);
    const Problem pb = problem_of(s, threshold, scale, vec);
    const long long *sd = p > 0.0 ? seed : nullptr;
    hipStream_t st = (hipStream_t)stream;
    const int rc = dispatch_kernel(dtype, pb.D, [&](auto t, auto tiles) {
        typedef type_of<decltype(t)> T;
        constexpr int CT = decltype(tiles)::value;
        hipLaunchKernelGGL((forward_kernel<T, CT>), grid, dim3(64), 0, st, (const T *)q, strides_of(*q_view), (const T *)k,
                           strides_of(*k_view), (const T *)v, strides_of(*v_view), sd, (T *)out, (float *)lse, (float *)out_acc, pb,
                           (int)s.N);
        return err.check_launch("selfattn_forward");
    });
    return rc == SELFATTN_OK ? 1 : rc;
}

int selfattn_backward(int dtype, const void *q, const selfattn_view *q_view, const void *k, const selfattn_view *k_view,
                      const void *v, const selfattn_view *v_view, const void *out_acc, const void *grad_out, const void *lse,
                      const long long *seed, double p, const selfattn_shape *shape, void *grad_q, void *grad_k, void *grad_v,
                      void *stream)
{
    err.clear();
    if (check_dtype(dtype) != SELFATTN_OK || check_shape(shape) != SELFATTN_OK) return SELFATTN_ERR_ARGUMENT;
    unsigned long long threshold;
    double scale;
    if (mask_of(p, seed, &threshold, &scale) != SELFATTN_OK) return SELFATTN_ERR_ARGUMENT;
    const selfattn_shape &s = *shape;
    if (!grad_q && !grad_k && !grad_v) return 0;
    if (s.L == 0 || s.N == 0 || s.S == 0) return 0;
    if (check_view(q_view, "q") != SELFATTN_OK || check_view(k_view, "k") != SELFATTN_OK || check_view(v_view, "v") != SELFATTN_OK)
        return SELFATTN_ERR_ARGUMENT;
    if (!q || !k || !v || !out_acc || !grad_out || !lse)
        return err.fail("null pointer: q, k, v, out_acc, grad_out and lse are required");
    dim3 grid_q, grid_kv;
    if (grid_of(s.L, s, &grid_q) != SELFATTN_OK || grid_of(s.S, s, &grid_kv) != SELFATTN_OK) return SELFATTN_ERR_ARGUMENT;
    const bool vec = aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out_acc) && aligned16(grad_out) && aligned16(grad_q) &&
                     aligned16(grad_k) && aligned16(grad_v) && quads(*q_view) && quads(*k_view) && quads(*v_view);
    const Problem pb = problem_of(s, threshold, scale, vec);
    const long long *sd = p > 0.0 ? seed : nullptr;
    hipStream_t st = (hipStream_t)stream;
    int launches = 0;
    const int rc = dispatch_kernel(dtype, pb.D, [&](auto t, auto tiles) {
        typedef type_of<decltype(t)> T;
        constexpr int CT = decltype(tiles)::value;
        if (grad_q) {
            hipLaunchKernelGGL((backward_q_kernel<T, CT>), grid_q, dim3(64), 0, st, (const T *)q, strides_of(*q_view),
                               (const T *)k, strides_of(*k_view), (const T *)v, strides_of(*v_view), (const float *)out_acc,
                               (const T *)grad_out, (const float *)lse, sd, (T *)grad_q, pb, (int)s.N);
            ++launches;
        }
        if (grad_k || grad_v) {
            hipLaunchKernelGGL((backward_kv_kernel<T, CT>), grid_kv, dim3(64), 0, st, (const T *)q, strides_of(*q_view),
                               (const T *)k, strides_of(*k_view), (const T *)v, strides_of(*v_view), (const float *)out_acc,
                               (const T *)grad_out, (const float *)lse, sd, (T *)grad_k, (T *)grad_v, pb, (int)s.N);
            ++launches;
        }
        return err.check_launch("selfattn_backward");
    });
    return rc == SELFATTN_OK ? launches : rc;
}

}  // extern "C"
