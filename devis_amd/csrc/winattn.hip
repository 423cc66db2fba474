// winattn.hip -- the Swin backbone's (shifted-)window attention between the qkv and proj Linears of a SwinTransformerBlock
// (include/winattn.h): cyclic shift, window partition, relative-position bias, shift mask, softmax, product
// with v, window merge and reverse shift as index arithmetic around one attention pass, forward and backward.  gfx950, wave64,
// plain HIP, the register map of selfattn.hip: one wave owns 16 tokens of one (b, window, head) and walks the window's other
// tokens in tiles of 16; the logit tile stays in the accumulator registers of v_mfma_f32_16x16x4_f32.  There is no LDS, no
// atomic and nothing is zeroed.  The unit is self-contained: it shares no code with selfattn.hip.
#include "op_common.h"       // (fp contraction off)
#include "winattn.h"

namespace winattn {

using namespace devis;

static_assert(WINATTN_OK == kOk && WINATTN_ERR_ARGUMENT == kErrArgument && WINATTN_ERR_HIP == kErrHip, "status codes");
static_assert(WINATTN_F32 == kF32 && WINATTN_F64 == kF64 && WINATTN_BF16 == kBF16 && WINATTN_F16 == kF16, "dtype codes");

constexpr int kTile = 16;                       // tokens of a wave, and tokens of a tile of the window
constexpr int kMaxD = WINATTN_MAX_HEAD_DIM;
constexpr int kMaxWindow = WINATTN_MAX_WINDOW;
constexpr float kMasked = -100.0f;              // the shift mask: finite and additive (include/winattn.h)

thread_local Status err;     // winattn_last_error()

typedef float f32x4 __attribute__((ext_vector_type(4)));

// D[i][j] += sum over the 4 k-slots of A[i][slot] * B[slot][j]: lane l gives A[l & 15][l >> 4] and B[l >> 4][l & 15] and
// holds D[4 * (l >> 4) + reg][l & 15]
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0); }

// the problem, as the kernels take it
struct Problem {
    int B, Hp, Wp, nH, D, ws, shift;
    int N, nWx, nW, QT;                         // tokens per window, windows per map row, per map, tiles of 16 tokens
    int magic;                                  // ceil(2^16 / ws): (i * magic) >> 16 == i / ws for every i < 2^16 / ws
    long long C;                                // nH * D
    float scale;
    int vec;                                    // every pointer 16-byte aligned
    int wide;                                   // the table is float32 beside a 16-bit storage dtype
};

// a token of a window: where it sits
struct Token {
    long long pixel;                            // (b * Hp + y) * Wp + x of its map pixel
    int iy, ix;                                 // inside the window
    int region;                                 // of the shift mask
};

// The wave's place: blockIdx.x = (bw * nH + h) * QT + tile with bw = b * nW + w
struct Place {
    int tile, h, b, wy, wx;
    long long bw;
};

__device__ __forceinline__ Place place_of(const Problem &pb, long long x)
{
    Place p;
    p.tile = (int)(x % pb.QT);
    x /= pb.QT;
    p.h = (int)(x % pb.nH);
    p.bw = x / pb.nH;
    p.b = (int)(p.bw / pb.nW);
    const int w = (int)(p.bw - (long long)p.b * pb.nW);
    p.wy = w / pb.nWx;
    p.wx = w - p.wy * pb.nWx;
    return p;
}

__device__ __forceinline__ void window_of(const Problem &pb, long long bw, int *b, int *wy, int *wx)
{
    *b = (int)(bw / pb.nW);
    const int w = (int)(bw - (long long)*b * pb.nW);
    *wy = w / pb.nWx;
    *wx = w - *wy * pb.nWx;
}

// token i of window (wy, wx) of batch entry b.  For i >= N the result is never dereferenced.
__device__ __forceinline__ Token token_of(const Problem &pb, int b, int wy, int wx, int i)
{
    Token t;
    t.iy = (i * pb.magic) >> 16;
    t.ix = i - t.iy * pb.ws;
    const int ys = wy * pb.ws + t.iy, xs = wx * pb.ws + t.ix;
    int y = ys + pb.shift, x = xs + pb.shift;
    if (y >= pb.Hp) y -= pb.Hp;
    if (x >= pb.Wp) x -= pb.Wp;
    t.pixel = ((long long)b * pb.Hp + y) * pb.Wp + x;
    t.region = 3 * ((ys >= pb.Hp - pb.ws) + (ys >= pb.Hp - pb.shift)) + (xs >= pb.Wp - pb.ws) + (xs >= pb.Wp - pb.shift);
    return t;
}

// table[(iy - jy + ws - 1) * (2 ws - 1) + (ix - jx + ws - 1), h] of query token qi and key token kj, both valid
template <typename T> __device__ __forceinline__ float bias_of(const Problem &pb, const void *table, int h, const Token &qi, const Token &kj)
{
    const int row = (qi.iy - kj.iy + pb.ws - 1) * (2 * pb.ws - 1) + (qi.ix - kj.ix + pb.ws - 1);
    const long long at = (long long)row * pb.nH + h;
    return pb.wide ? static_cast<const float *>(table)[at] : to_acc(static_cast<const T *>(table)[at]);
}

// mask(i, j); -inf for a key that does not exist, so that its logit is -inf and its probability 0
__device__ __forceinline__ float mask_of(const Problem &pb, const Token &qi, const Token &kj, bool valid)
{
    if (!valid) return -INFINITY;
    return pb.shift > 0 && qi.region != kj.region ? kMasked : 0.0f;
}

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
// Wave blockIdx.x: the queries [16 * tile, ...) of head h of window bw.  CT tiles of 16 channels cover a head.
template <typename T, int CT>
__global__ __launch_bounds__(64) void forward_kernel(const T *__restrict__ qkv, const void *__restrict__ table, T *__restrict__ out,
                                                     float *__restrict__ lse, float *__restrict__ out_acc, const Problem pb)
{
    constexpr int NQ = 4 * CT;
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const Place at = place_of(pb, blockIdx.x);
    const int N = pb.N, D = pb.D, n = D >> 2, h = at.h;
    const int i = at.tile * kTile + c;
    const bool chunk_vec = pb.vec && (n & 3) == 0;
    const long long C = pb.C, C3 = 3 * pb.C, head = (long long)h * D;
    const Token qi = token_of(pb, at.b, at.wy, at.wx, i);
    float qf[NQ];
    load_chunk<T, NQ>(qkv + qi.pixel * C3 + head + g * n, n, i < N, chunk_vec, qf);
    f32x4 o[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) o[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float m = -INFINITY, l = 0.0f;                  // of query c: the maximum so far, this lane's share of the sum
    // the operands of the tile at j0: this lane's chunk of key j0 + c; channel ct * 16 + c of the keys j0 + 4 g + r, their bias
    // and their mask
    auto load_tile = [&](int j0, float (&kf)[NQ], float (&vt)[CT][4], float (&bias)[4], float (&mask)[4]) {
        const Token kc = token_of(pb, at.b, at.wy, at.wx, j0 + c);
        load_chunk<T, NQ>(qkv + kc.pixel * C3 + C + head + g * n, n, j0 + c < N, chunk_vec, kf);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + 4 * g + r;
            const Token kj = token_of(pb, at.b, at.wy, at.wx, j);
            const bool both = j < N && i < N;
            bias[r] = both ? bias_of<T>(pb, table, h, qi, kj) : 0.0f;
            mask[r] = mask_of(pb, qi, kj, j < N);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
                vt[ct][r] = load_one(qkv + kj.pixel * C3 + 2 * C + head + ct * 16 + c, ct * 16 + c < D && j < N);
        }
    };
    float kf[NQ], vt[CT][4], bias[4], mask[4];
    load_tile(0, kf, vt, bias, mask);
    for (int j0 = 0; j0 < N; j0 += kTile) {
        float k_next[NQ], v_next[CT][4], bias_next[4], mask_next[4];       // the next tile is in flight while this one is computed
        load_tile(j0 + kTile, k_next, v_next, bias_next, mask_next);
        const f32x4 st = dot_tile<NQ>(kf, qf, n);   // S^T: register r is key j0 + 4 g + r, the lane column query c
        float s[4], tile_max = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[r] = (st[r] * pb.scale + bias[r]) + mask[r];
            tile_max = fmaxf(tile_max, s[r]);
        }
        const float m_new = fmaxf(m, column_max(tile_max));
        const float alpha = expf(m - m_new);
        float pd[4], sum = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pd[r] = expf(s[r] - m_new);
            sum += pd[r];
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
        for (int r = 0; r < 4; ++r) {
            bias[r] = bias_next[r];
            mask[r] = mask_next[r];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) vt[ct][r] = v_next[ct][r];
        }
    }
    const float total = column_sum(l);
    if (i >= N) return;
    if (lse && g == 0) lse[(at.bw * pb.nH + h) * N + i] = m + logf(total);
    const float inv = 1.0f / total;
    const long long dense = qi.pixel * C + head;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int d0 = ct * 16 + 4 * g;             // register r is channel d0 + r
        if (d0 >= D) continue;
        store_quad(out + dense + d0, pb.vec != 0, o[ct], inv);
        if (out_acc) store_quad(out_acc + dense + d0, pb.vec != 0, o[ct], inv);       // before the rounding to T: the backward's
    }
}

// ---- backward: part 0 of grad_qkv (grad_q) ------------------------------------------------------------------------------------
// The forward's geometry.  P^T is recomputed from lse, dP^T = V dO^T lands in its layout, and dS^T is the B operand of
// dQ^T += K^T dS^T.
template <typename T, int CT>
__global__ __launch_bounds__(64) void backward_q_kernel(const T *__restrict__ qkv, const void *__restrict__ table,
                                                        const float *__restrict__ out, const T *__restrict__ grad_out,
                                                        const float *__restrict__ lse, T *__restrict__ grad_qkv, const Problem pb)
{
    constexpr int NQ = 4 * CT;
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const Place at = place_of(pb, blockIdx.x);
    const int N = pb.N, D = pb.D, n = D >> 2, h = at.h;
    const int i = at.tile * kTile + c;
    const bool chunk_vec = pb.vec && (n & 3) == 0;
    const long long C = pb.C, C3 = 3 * pb.C, head = (long long)h * D;
    const Token qi = token_of(pb, at.b, at.wy, at.wx, i);
    const long long dense = qi.pixel * C + head;                // of out and grad_out
    float qf[NQ], dof[NQ], of[NQ];
    load_chunk<T, NQ>(qkv + qi.pixel * C3 + head + g * n, n, i < N, chunk_vec, qf);
    load_chunk<T, NQ>(grad_out + dense + g * n, n, i < N, chunk_vec, dof);
    load_chunk<float, NQ>(out + dense + g * n, n, i < N, chunk_vec, of);
    const float delta = delta_of<NQ>(dof, of, n);
    const float lse_i = i < N ? lse[(at.bw * pb.nH + h) * N + i] : 0.0f;
    f32x4 dq[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) dq[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    // the operands of the tile at j0: this lane's chunks of key j0 + c; channel ct * 16 + c of the keys j0 + 4 g + r, their bias
    // and their mask
    auto load_tile = [&](int j0, float (&kf)[NQ], float (&vf)[NQ], float (&kt)[CT][4], float (&bias)[4], float (&mask)[4]) {
        const Token kc = token_of(pb, at.b, at.wy, at.wx, j0 + c);
        load_chunk<T, NQ>(qkv + kc.pixel * C3 + C + head + g * n, n, j0 + c < N, chunk_vec, kf);
        load_chunk<T, NQ>(qkv + kc.pixel * C3 + 2 * C + head + g * n, n, j0 + c < N, chunk_vec, vf);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + 4 * g + r;
            const Token kj = token_of(pb, at.b, at.wy, at.wx, j);
            const bool both = j < N && i < N;
            bias[r] = both ? bias_of<T>(pb, table, h, qi, kj) : 0.0f;
            mask[r] = mask_of(pb, qi, kj, j < N);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
                kt[ct][r] = load_one(qkv + kj.pixel * C3 + C + head + ct * 16 + c, ct * 16 + c < D && j < N);
        }
    };
    float kf[NQ], vf[NQ], kt[CT][4], bias[4], mask[4];
    load_tile(0, kf, vf, kt, bias, mask);
    for (int j0 = 0; j0 < N; j0 += kTile) {
        float k_next[NQ], v_next[NQ], kt_next[CT][4], bias_next[4], mask_next[4];
        load_tile(j0 + kTile, k_next, v_next, kt_next, bias_next, mask_next);
        const f32x4 st = dot_tile<NQ>(kf, qf, n);
        const f32x4 dpt = dot_tile<NQ>(vf, dof, n);
        float ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float prob = expf(((st[r] * pb.scale + bias[r]) + mask[r]) - lse_i);
            ds[r] = prob * (dpt[r] - delta);
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
        for (int r = 0; r < 4; ++r) {
            bias[r] = bias_next[r];
            mask[r] = mask_next[r];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) kt[ct][r] = kt_next[ct][r];
        }
    }
    if (i >= N) return;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int d0 = ct * 16 + 4 * g;
        if (d0 < D) store_quad(grad_qkv + qi.pixel * C3 + head + d0, pb.vec != 0, dq[ct], pb.scale);
    }
}

// ---- backward: parts 1 and 2 of grad_qkv (grad_k and grad_v) --------------------------------------------------------------------
// Wave blockIdx.x: the keys [16 * tile, ...), walking the queries.  The tile is untransposed -- register r is query
// i0 + 4 g + r, the lane column key c --, so that it is the B operand of dV^T += dO^T P and dK^T += Q^T dS.
template <typename T, int CT>
__global__ __launch_bounds__(64) void backward_kv_kernel(const T *__restrict__ qkv, const void *__restrict__ table,
                                                         const float *__restrict__ out, const T *__restrict__ grad_out,
                                                         const float *__restrict__ lse, T *__restrict__ grad_qkv, const Problem pb)
{
    constexpr int NQ = 4 * CT;
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const Place at = place_of(pb, blockIdx.x);
    const int N = pb.N, D = pb.D, n = D >> 2, h = at.h;
    const int j = at.tile * kTile + c;
    const bool chunk_vec = pb.vec && (n & 3) == 0;
    const long long C = pb.C, C3 = 3 * pb.C, head = (long long)h * D;
    const Token kj = token_of(pb, at.b, at.wy, at.wx, j);
    const float *lse_w = lse + (at.bw * pb.nH + h) * N;
    float kf[NQ], vf[NQ];
    load_chunk<T, NQ>(qkv + kj.pixel * C3 + C + head + g * n, n, j < N, chunk_vec, kf);
    load_chunk<T, NQ>(qkv + kj.pixel * C3 + 2 * C + head + g * n, n, j < N, chunk_vec, vf);
    f32x4 dk[CT], dv[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) dk[ct] = dv[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int i0 = 0; i0 < N; i0 += kTile) {
        const int ic = i0 + c;                      // the query whose chunks this lane loads
        const Token qc = token_of(pb, at.b, at.wy, at.wx, ic);
        const long long dense = qc.pixel * C + head;
        float qf[NQ], dof[NQ], of[NQ];
        load_chunk<T, NQ>(qkv + qc.pixel * C3 + head + g * n, n, ic < N, chunk_vec, qf);
        load_chunk<T, NQ>(grad_out + dense + g * n, n, ic < N, chunk_vec, dof);
        load_chunk<float, NQ>(out + dense + g * n, n, ic < N, chunk_vec, of);
        const f32x4 st = dot_tile<NQ>(qf, kf, n);
        const f32x4 dpt = dot_tile<NQ>(dof, vf, n);
        const float delta_c = delta_of<NQ>(dof, of, n);                 // of query i0 + c
        float prob[4], ds[4];
        long long q_pixel[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 4 * g + r;
            const Token qi = token_of(pb, at.b, at.wy, at.wx, i);
            q_pixel[r] = qi.pixel;
            const bool both = i < N && j < N;
            const float bias = both ? bias_of<T>(pb, table, h, qi, kj) : 0.0f;
            const float mask = mask_of(pb, qi, kj, both);
            prob[r] = both ? expf(((st[r] * pb.scale + bias) + mask) - lse_w[i]) : 0.0f;
            const float delta = __shfl(delta_c, 4 * g + r, 64);         // of query i0 + 4 g + r
            ds[r] = prob[r] * (dpt[r] - delta);
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            if (ct * 16 >= D) continue;
            const bool channel = ct * 16 + c < D;
#pragma unroll
            for (int r = 0; r < 4; ++r) {           // k-slot g of step r is query i0 + 4 g + r
                const bool valid = channel && i0 + 4 * g + r < N;
                const float a_v = load_one(grad_out + q_pixel[r] * C + head + ct * 16 + c, valid);
                dv[ct] = mfma4(a_v, prob[r], dv[ct]);                   // dV^T += dO^T P
                const float a_k = load_one(qkv + q_pixel[r] * C3 + head + ct * 16 + c, valid);
                dk[ct] = mfma4(a_k, ds[r], dk[ct]);                     // dK^T += Q^T dS
            }
        }
    }
    if (j >= N) return;
    const long long dst = kj.pixel * C3 + head;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int d0 = ct * 16 + 4 * g;
        if (d0 >= D) continue;
        store_quad(grad_qkv + dst + C + d0, pb.vec != 0, dk[ct], pb.scale);
        store_quad(grad_qkv + dst + 2 * C + d0, pb.vec != 0, dv[ct], 1.0f);
    }
}

// ---- backward: grad_table -------------------------------------------------------------------------------------------------------
// Wave blockIdx.x = ((chunk * nH + h) * QT + query tile) * QT + key tile: the sum of dS^T of that tile pair over the windows
// [chunk * per, ...) in ascending order -> partial [chunks, nH, N, N].
template <typename T, int CT>
__global__ __launch_bounds__(64) void backward_bias_kernel(const T *__restrict__ qkv, const void *__restrict__ table,
                                                           const float *__restrict__ out, const T *__restrict__ grad_out,
                                                           const float *__restrict__ lse, float *__restrict__ partial,
                                                           const Problem pb, const long long per, const long long windows)
{
    constexpr int NQ = 4 * CT;
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    long long x = blockIdx.x;
    const int key_tile = (int)(x % pb.QT);
    x /= pb.QT;
    const int query_tile = (int)(x % pb.QT);
    x /= pb.QT;
    const int h = (int)(x % pb.nH);
    const long long chunk = x / pb.nH;
    const int N = pb.N, D = pb.D, n = D >> 2;
    const int i = query_tile * kTile + c, j0 = key_tile * kTile;
    const bool chunk_vec = pb.vec && (n & 3) == 0;
    const long long C = pb.C, C3 = 3 * pb.C, head = (long long)h * D;
    const long long first = chunk * per, last = first + per < windows ? first + per : windows;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (long long bw = first; bw < last; ++bw) {
        int b, wy, wx;
        window_of(pb, bw, &b, &wy, &wx);
        const Token qi = token_of(pb, b, wy, wx, i);
        const Token kc = token_of(pb, b, wy, wx, j0 + c);
        const long long dense = qi.pixel * C + head;
        float qf[NQ], dof[NQ], of[NQ], kf[NQ], vf[NQ];
        load_chunk<T, NQ>(qkv + qi.pixel * C3 + head + g * n, n, i < N, chunk_vec, qf);
        load_chunk<T, NQ>(grad_out + dense + g * n, n, i < N, chunk_vec, dof);
        load_chunk<float, NQ>(out + dense + g * n, n, i < N, chunk_vec, of);
        load_chunk<T, NQ>(qkv + kc.pixel * C3 + C + head + g * n, n, j0 + c < N, chunk_vec, kf);
        load_chunk<T, NQ>(qkv + kc.pixel * C3 + 2 * C + head + g * n, n, j0 + c < N, chunk_vec, vf);
        const float delta = delta_of<NQ>(dof, of, n);
        const float lse_i = i < N ? lse[(bw * pb.nH + h) * N + i] : 0.0f;
        const f32x4 st = dot_tile<NQ>(kf, qf, n);
        const f32x4 dpt = dot_tile<NQ>(vf, dof, n);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + 4 * g + r;
            const Token kj = token_of(pb, b, wy, wx, j);
            const bool both = i < N && j < N;
            const float bias = both ? bias_of<T>(pb, table, h, qi, kj) : 0.0f;
            const float mask = mask_of(pb, qi, kj, both);
            const float prob = both ? expf(((st[r] * pb.scale + bias) + mask) - lse_i) : 0.0f;
            acc[r] += prob * (dpt[r] - delta);
        }
    }
    if (i >= N) return;
    float *dst = partial + ((chunk * pb.nH + h) * N + i) * N;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = j0 + 4 * g + r;
        if (j < N) dst[j] = acc[r];
    }
}

// partial [chunks, count] -> total [count]: the chunks in ascending order
__global__ __launch_bounds__(256) void reduce_chunks_kernel(const float *__restrict__ partial, float *__restrict__ total,
                                                            const long long count, const long long chunks)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    float s = partial[t];
    for (long long k = 1; k < chunks; ++k) s += partial[k * count + t];
    total[t] = s;
}

// total [nH, N, N] -> grad_table [(2 ws - 1)^2, nH]: every (i, j) whose table row is r, in ascending (i, j)
template <typename TB>
__global__ __launch_bounds__(256) void fold_kernel(const float *__restrict__ total, TB *__restrict__ grad_table, const Problem pb)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int side = 2 * pb.ws - 1;
    if (t >= side * side * pb.nH) return;
    const int h = t % pb.nH, row = t / pb.nH;
    const int dy = row / side - (pb.ws - 1), dx = row % side - (pb.ws - 1);          // iy - jy, ix - jx
    const int iy_lo = dy > 0 ? dy : 0, iy_hi = dy > 0 ? pb.ws : pb.ws + dy;
    const int ix_lo = dx > 0 ? dx : 0, ix_hi = dx > 0 ? pb.ws : pb.ws + dx;
    const float *src = total + (long long)h * pb.N * pb.N;
    float s = 0.0f;
    for (int iy = iy_lo; iy < iy_hi; ++iy)
        for (int ix = ix_lo; ix < ix_hi; ++ix) {
            const int i = iy * pb.ws + ix, j = (iy - dy) * pb.ws + (ix - dx);
            s += src[(long long)i * pb.N + j];
        }
    from_acc(grad_table[t], s);
}

// ---- host -------------------------------------------------------------------------------------------------------------------
constexpr long long kMax31 = 0x7fffffffLL;
constexpr long long kTargetWaves = 16384, kMaxChunks = 256;
constexpr long long kMaxBlocks = (1LL << 26) - 1;

int check_shape(const winattn_shape *s)
{
    if (!s) return err.fail("null pointer: shape");
    if (s->B < 0 || s->Hp < 0 || s->Wp < 0) return err.fail("B, Hp and Wp must not be negative");
    if (s->B > kMax31 || s->Hp > kMax31 || s->Wp > kMax31) return err.fail("B, Hp and Wp must fit 31 bits (Hp = %lld, Wp = %lld)", s->Hp, s->Wp);
    if (s->heads < 1 || s->heads > 65535) return err.fail("the number of heads must be in [1, 65535], got %lld", s->heads);
    if (s->head_dim % 4 || s->head_dim < 4 || s->head_dim > kMaxD)
        return err.fail("the head dimension must be a multiple of 4 in [4, %lld], got %lld", (long long)kMaxD, s->head_dim);
    if (s->window < 1 || s->window > kMaxWindow)
        return err.fail("the window size must be in [1, %lld], got %lld", (long long)kMaxWindow, s->window);
    if (s->shift < 0 || s->shift >= s->window) return err.fail("the shift must be in [0, window), got %lld beside a window of %lld", s->shift, s->window);
    if (s->Hp % s->window || s->Wp % s->window)
        return err.fail("Hp = %lld and Wp = %lld must be multiples of the window size", s->Hp, s->Wp);
    if (s->Hp * s->Wp > kMax31 || s->B * (s->Hp * s->Wp) > kMax31) return err.fail("B * Hp * Wp does not fit 31 bits");
    return WINATTN_OK;
}

int check_dtype(int dtype)
{
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (dtype == kF64) return err.fail("unsupported dtype: float64 (float32, bfloat16 or float16)");
    return WINATTN_OK;
}

int check_scale(double scale)
{
    if (!(scale == scale) || scale - scale != 0.0) return err.fail("scale must be finite");
    return WINATTN_OK;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }       // (NULL is aligned)

bool empty(const winattn_shape &s) { return s.B == 0 || s.Hp == 0 || s.Wp == 0; }

Problem problem_of(const winattn_shape &s, double scale, bool vec, int wide)
{
    Problem pb;
    pb.B = (int)s.B;
    pb.Hp = (int)s.Hp;
    pb.Wp = (int)s.Wp;
    pb.nH = (int)s.heads;
    pb.D = (int)s.head_dim;
    pb.ws = (int)s.window;
    pb.shift = (int)s.shift;
    pb.N = pb.ws * pb.ws;
    pb.nWx = pb.Wp / pb.ws;
    pb.nW = (pb.Hp / pb.ws) * pb.nWx;
    pb.QT = (pb.N + kTile - 1) / kTile;
    pb.magic = (65536 + pb.ws - 1) / pb.ws;
    pb.C = s.heads * s.head_dim;
    pb.scale = (float)scale;
    pb.vec = vec ? 1 : 0;
    pb.wide = wide ? 1 : 0;
    return pb;
}

// how grad_table's first pass splits the B * nW windows: a function of the shape alone
void chunks_of(const winattn_shape &s, long long *chunks, long long *per)
{
    const long long N = s.window * s.window, QT = cdiv(N, kTile);
    const long long windows = s.B * (s.Hp / s.window) * (s.Wp / s.window);
    long long want = cdiv(kTargetWaves, QT * QT * s.heads);
    if (want > kMaxChunks) want = kMaxChunks;
    if (want > windows) want = windows;
    if (want < 1) want = 1;
    *per = windows ? cdiv(windows, want) : 1;
    *chunks = windows ? cdiv(windows, *per) : 1;
}

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

// `blocks` workgroups of 64 threads: a launch takes fewer than 2^32 threads
int grid_of(long long blocks, unsigned *x)
{
    if (blocks > kMaxBlocks) return err.fail("too many workgroups for one launch (%lld, at most %lld)", blocks, kMaxBlocks);
    *x = (unsigned)blocks;
    return WINATTN_OK;
}

// one wave per (window, head, tile of 16 tokens)
int grid_of(const Problem &pb, unsigned *x) { return grid_of((long long)pb.B * pb.nW * pb.nH * pb.QT, x); }

}  // namespace winattn

using namespace winattn;

extern "C" {

int winattn_version(void) { return WINATTN_ABI_VERSION; }

const char *winattn_last_error(void) { return err.msg; }

long long winattn_workspace_bytes(const winattn_shape *shape)
{
    err.clear();
    if (check_shape(shape) != WINATTN_OK) return WINATTN_ERR_ARGUMENT;
    long long chunks, per;
    chunks_of(*shape, &chunks, &per);
    const long long N = shape->window * shape->window;
    return (chunks + 1) * shape->heads * N * N * (long long)sizeof(float);
}

int winattn_forward(int dtype, int wide, const void *qkv, const void *bias_table, double scale, const winattn_shape *shape,
                    void *out, void *lse, void *out_acc, void *stream)
{
    err.clear();
    if (check_dtype(dtype) != WINATTN_OK || check_shape(shape) != WINATTN_OK || check_scale(scale) != WINATTN_OK)
        return WINATTN_ERR_ARGUMENT;
    if (wide && dtype == kF32) wide = 0;
    const winattn_shape &s = *shape;
    if (empty(s)) return 0;
    if (!qkv || !bias_table || !out) return err.fail("null pointer: qkv, bias_table and out are required");
    const bool vec = aligned16(qkv) && aligned16(out) && aligned16(out_acc);
    const Problem pb = problem_of(s, scale, vec, wide);
    unsigned grid;
    if (grid_of(pb, &grid) != WINATTN_OK) return WINATTN_ERR_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    const int rc = dispatch_kernel(dtype, pb.D, [&](auto t, auto tiles) {
        typedef type_of<decltype(t)> T;
        constexpr int CT = decltype(tiles)::value;
        hipLaunchKernelGGL((forward_kernel<T, CT>), dim3(grid), dim3(64), 0, st, (const T *)qkv, bias_table, (T *)out, (float *)lse,
                           (float *)out_acc, pb);
        return err.check_launch("winattn_forward");
    });
    return rc == WINATTN_OK ? 1 : rc;
}

int winattn_backward(int dtype, int wide, const void *qkv, const void *bias_table, const void *out_acc, const void *grad_out,
                     const void *lse, double scale, const winattn_shape *shape, void *grad_qkv, void *grad_table,
                     void *workspace, void *stream)
{
    err.clear();
    if (check_dtype(dtype) != WINATTN_OK || check_shape(shape) != WINATTN_OK || check_scale(scale) != WINATTN_OK)
        return WINATTN_ERR_ARGUMENT;
    if (wide && dtype == kF32) wide = 0;
    const winattn_shape &s = *shape;
    if (!grad_qkv && !grad_table) return 0;
    if (empty(s)) return 0;
    if (!qkv || !bias_table || !out_acc || !grad_out || !lse)
        return err.fail("null pointer: qkv, bias_table, out_acc, grad_out and lse are required");
    if (grad_table && !workspace) return err.fail("null pointer: a workspace is required with grad_table");
    if (((uintptr_t)workspace & 3) != 0) return err.fail("the workspace must be 4-byte aligned");
    const bool vec = aligned16(qkv) && aligned16(out_acc) && aligned16(grad_out) && aligned16(grad_qkv);
    const Problem pb = problem_of(s, scale, vec, wide);
    unsigned grid, grid_bias = 0;
    if (grid_of(pb, &grid) != WINATTN_OK) return WINATTN_ERR_ARGUMENT;
    long long chunks, per;
    chunks_of(s, &chunks, &per);
    if (grad_table && grid_of(chunks * pb.nH * pb.QT * pb.QT, &grid_bias) != WINATTN_OK) return WINATTN_ERR_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    int launches = 0;
    const int rc = dispatch_kernel(dtype, pb.D, [&](auto t, auto tiles) {
        typedef type_of<decltype(t)> T;
        constexpr int CT = decltype(tiles)::value;
        if (grad_qkv) {
            hipLaunchKernelGGL((backward_q_kernel<T, CT>), dim3(grid), dim3(64), 0, st, (const T *)qkv, bias_table,
                               (const float *)out_acc, (const T *)grad_out, (const float *)lse, (T *)grad_qkv, pb);
            hipLaunchKernelGGL((backward_kv_kernel<T, CT>), dim3(grid), dim3(64), 0, st, (const T *)qkv, bias_table,
                               (const float *)out_acc, (const T *)grad_out, (const float *)lse, (T *)grad_qkv, pb);
            launches += 2;
        }
        if (grad_table) {
            const long long count = (long long)pb.nH * pb.N * pb.N;
            float *partial = (float *)workspace, *total = partial + chunks * count;
            hipLaunchKernelGGL((backward_bias_kernel<T, CT>), dim3(grid_bias), dim3(64), 0, st, (const T *)qkv, bias_table,
                               (const float *)out_acc, (const T *)grad_out, (const float *)lse, partial, pb, per,
                               (long long)pb.B * pb.nW);
            hipLaunchKernelGGL(reduce_chunks_kernel, dim3((unsigned)cdiv(count, 256)), dim3(256), 0, st, partial, total, count, chunks);
            const int side = 2 * pb.ws - 1;
            const dim3 fold_grid((unsigned)cdiv((long long)side * side * pb.nH, 256));
            if (wide)
                hipLaunchKernelGGL((fold_kernel<float>), fold_grid, dim3(256), 0, st, total, (float *)grad_table, pb);
            else
                hipLaunchKernelGGL((fold_kernel<T>), fold_grid, dim3(256), 0, st, total, (T *)grad_table, pb);
            launches += 3;
        }
        return err.check_launch("winattn_backward");
    });
    return rc == WINATTN_OK ? launches : rc;
}

}  // extern "C"
