// swinends.hip -- the two ends of the Swin backbone (include/swinends.h): the patch embedding -- zero
// padding, p x p / stride-p projection and LayerNorm written straight into token order -- and the per-stage output norm written
// straight into the NCHW map, forward and backward.  gfx950, wave64, plain HIP.  A workgroup owns a tile of 32 consecutive
// tokens, a wave 8 of them; the row of a token lives in a wave's registers and is norm_row.h's, as in prenorm.hip.
#include "op_common.h"       // (fp contraction off; devis::normrow, the row of norm_row.h)
#include "swinends.h"

namespace swinends {

using namespace devis;
using namespace devis::normrow;

static_assert(SWINENDS_OK == kOk && SWINENDS_ERR_ARGUMENT == kErrArgument && SWINENDS_ERR_HIP == kErrHip, "status codes");
static_assert(SWINENDS_F32 == kF32 && SWINENDS_BF16 == kBF16 && SWINENDS_F16 == kF16, "dtype codes");

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 32;                   // tokens of a workgroup's tile
constexpr int kWaveRows = kTile / kWaves;   // tokens of a wave
constexpr int kEmbedChunk = 512;            // tokens of a chunk of the embedding backward's sums
constexpr int kChunkTiles = kEmbedChunk / kTile;
constexpr int kMaxK = SWINENDS_MAX_PATCH;
constexpr int kMaxEmbed = SWINENDS_MAX_EMBED;
constexpr int kMaxC = SWINENDS_MAX_CHANNELS;
constexpr int kSlice = kTile * kSpan;       // floats of the weight slice of the embedding (32 KiB); also its [32][256] dz tile
constexpr int kPitch = kTile + 1;           // floats of a row of the map's [256][32] LDS tile: odd, so the 64 deposits of a wave
                                            // (rows 64 j + l) and the 32 reads along a row each fall into distinct banks
static_assert(kWaveRows == 8 && kSlice >= kWaves * 3 * kSpan, "a wave reads its 8 patch values as two float4");

thread_local Status err;     // swinends_last_error()

struct EGeo {
    long long R;            // tokens
    long long HpWp;
    int Cin, H, W, p, C, K, Hp, Wp;
};

struct MGeo {
    long long R;            // rows
    long long HW;
    int C;
};

// ---- the embedding: what forward and backward share --------------------------------------------------------------------------
// the patches of the tile's tokens -> patchT [K][kTile], a pixel outside H x W and a token >= R as 0.  Consecutive threads read
// consecutive pixels of an image row across the tile's tokens.
template <typename TI> __device__ __forceinline__ void stage_patches(const TI *__restrict__ image, const EGeo &geo, long long tile0,
                                                                      float *patchT)
{
    const int p = geo.p, run = kTile * p, total = geo.Cin * p * run;
    for (int e = threadIdx.x; e < total; e += kThreads) {
        const int cd = e / run, rest = e - cd * run;         // cd = cin * p + dy
        const int t = rest / p, dx = rest - t * p;
        const int cin = cd / p, dy = cd - cin * p;
        const long long n = tile0 + t;
        float v = 0.0f;
        if (n < geo.R) {
            const long long b = n / geo.HpWp, rem = n - b * geo.HpWp;
            const int i = (int)(rem / geo.Wp), j = (int)(rem - (long long)i * geo.Wp);
            const int y = i * p + dy, x = j * p + dx;
            if (y < geo.H && x < geo.W) v = to_acc(image[((b * geo.Cin + cin) * geo.H + y) * (long long)geo.W + x]);
        }
        patchT[(cd * p + dx) * kTile + t] = v;
    }
}

// z of the wave's 8 tokens: the fma chain over k ascending, then the bias.  The weight goes through LDS in slices of KC values
// of k, transposed to [k][CP].  Begins with a barrier (the patches are staged, `slice` is free).
template <typename TP, int G>
__device__ __forceinline__ void project(const TP *__restrict__ proj_weight, const TP *__restrict__ proj_bias, const EGeo &geo,
                                        const float *patchT, float *slice, float (&z)[kWaveRows][G][4])
{
    constexpr int CP = G * kSpan + 4;       // (+ 4: the staging writes of consecutive k spread over banks; rows stay 16-byte aligned)
    constexpr int KC = kSlice / CP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, C = geo.C, K = geo.K;
#pragma unroll
    for (int r = 0; r < kWaveRows; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int j = 0; j < 4; ++j) z[r][g][j] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += KC) {
        const int kc = K - k0 < KC ? K - k0 : KC;
        __syncthreads();
        for (int e = threadIdx.x; e < G * kSpan * kc; e += kThreads) {
            const int c = e / kc, kk = e - c * kc;
            slice[kk * CP + c] = c < C ? to_acc(proj_weight[(long long)c * K + k0 + kk]) : 0.0f;
        }
        __syncthreads();
        for (int kk = 0; kk < kc; ++kk) {
            const float4 pa = *reinterpret_cast<const float4 *>(patchT + (k0 + kk) * kTile + wave * kWaveRows);
            const float4 pb = *reinterpret_cast<const float4 *>(patchT + (k0 + kk) * kTile + wave * kWaveRows + 4);
            const float pv[kWaveRows] = {pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, pb.z, pb.w};
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float4 w = *reinterpret_cast<const float4 *>(slice + kk * CP + g * kSpan + lane * 4);
                const float wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int r = 0; r < kWaveRows; ++r)
#pragma unroll
                    for (int j = 0; j < 4; ++j) z[r][g][j] = fmaf(wv[j], pv[r], z[r][g][j]);
            }
        }
    }
    if (proj_bias) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int c0 = channel_of(g, lane);
            float b[4];
            load4(proj_bias + c0, C - c0, false, b);
#pragma unroll
            for (int r = 0; r < kWaveRows; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) z[r][g][j] = z[r][g][j] + b[j];
        }
    }
}

// ---- the embedding, forward --------------------------------------------------------------------------------------------------
template <typename TI, typename TP, typename TY, int G>
__global__ __launch_bounds__(kThreads) void embed_forward_kernel(const TI *__restrict__ image, const TP *__restrict__ proj_weight,
                                                                 const TP *__restrict__ proj_bias, const TP *__restrict__ norm_weight,
                                                                 const TP *__restrict__ norm_bias, TY *__restrict__ tokens,
                                                                 float *__restrict__ mean_out, float *__restrict__ rstd_out,
                                                                 const EGeo geo, const float eps, const int vec_)
{
    __shared__ __attribute__((aligned(16))) float patchT[kMaxK * kTile];
    __shared__ __attribute__((aligned(16))) float slice[kSlice];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, C = geo.C;
    const bool vec = vec_ != 0;
    const long long tile0 = (long long)blockIdx.x * kTile;
    stage_patches(image, geo, tile0, patchT);
    float z[kWaveRows][G][4];
    project<TP, G>(proj_weight, proj_bias, geo, patchT, slice, z);
    float nw[G][4], nb[G][4];
    if (norm_weight) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int c0 = channel_of(g, lane);
            load4(norm_weight + c0, C - c0, false, nw[g]);
            load4(norm_bias + c0, C - c0, false, nb[g]);
        }
    }
#pragma unroll
    for (int r = 0; r < kWaveRows; ++r) {
        const long long n = tile0 + wave * kWaveRows + r;
        if (n >= geo.R) break;
        if (norm_weight) {
            const float mean = row_sum<G>(z[r], C, lane) / (float)C;
            float sq[G][4];
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float t = z[r][g][j] - mean;
                    sq[g][j] = t * t;
                }
            const float var = row_sum<G>(sq, C, lane) / (float)C;
            const float rstd = rsqrt_of(var + eps);
            if (mean_out && lane == 0) {
                mean_out[n] = mean;
                rstd_out[n] = rstd;
            }
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j) z[r][g][j] = ((z[r][g][j] - mean) * rstd) * nw[g][j] + nb[g][j];
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int c0 = channel_of(g, lane);
            store4(tokens + n * C + c0, C - c0, vec, z[r][g]);
        }
    }
}

// ---- the embedding, backward -------------------------------------------------------------------------------------------------
// Workgroup `chunk` owns the tokens [chunk * kEmbedChunk, ...), tile after tile: z again, dz, the column sums of the chunk in
// registers and the chunk's partial of grad_proj_weight in the workspace.
//   ws_cols [chunks][3][C]: g * xhat, g, dz.      ws_w [chunks][K][C].
template <typename TI, typename TP, typename TY, int G>
__global__ __launch_bounds__(kThreads) void embed_backward_kernel(const TI *__restrict__ image, const TP *__restrict__ proj_weight,
                                                                  const TP *__restrict__ proj_bias, const TP *__restrict__ norm_weight,
                                                                  const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                  const TY *__restrict__ grad_tokens, float *__restrict__ ws_cols,
                                                                  float *__restrict__ ws_w, const EGeo geo, const int vec_)
{
    __shared__ __attribute__((aligned(16))) float patchT[kMaxK * kTile];
    __shared__ __attribute__((aligned(16))) float slice[kSlice];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, C = geo.C, K = geo.K;
    const bool vec = vec_ != 0;
    const long long chunk = blockIdx.x;
    float nw[G][4], sum_w[G][4], sum_b[G][4], sum_z[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c0 = channel_of(g, lane);
        if (norm_weight) load4(norm_weight + c0, C - c0, false, nw[g]);
#pragma unroll
        for (int j = 0; j < 4; ++j) sum_w[g][j] = sum_b[g][j] = sum_z[g][j] = 0.0f;
    }
    for (int tile = 0; tile < kChunkTiles; ++tile) {
        const long long tile0 = chunk * kEmbedChunk + (long long)tile * kTile;
        if (tile0 >= geo.R) break;
        __syncthreads();                                    // (the last tile's patches and dz tile are read)
        stage_patches(image, geo, tile0, patchT);
        float z[kWaveRows][G][4];
        project<TP, G>(proj_weight, proj_bias, geo, patchT, slice, z);
#pragma unroll
        for (int r = 0; r < kWaveRows; ++r) {               // z[r] becomes dz, 0 for a token >= R
            const long long n = tile0 + wave * kWaveRows + r;
            if (n >= geo.R) {
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) z[r][g][j] = 0.0f;
                continue;
            }
            float gy[G][4];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int c0 = channel_of(g, lane);
                load4(grad_tokens + n * C + c0, C - c0, vec, gy[g]);
            }
            if (norm_weight) {
                const float m = mean[n], rs = rstd[n];
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        z[r][g][j] = (z[r][g][j] - m) * rs;         // xhat, the forward's bits
                        sum_w[g][j] += gy[g][j] * z[r][g][j];
                        sum_b[g][j] += gy[g][j];
                        gy[g][j] = gy[g][j] * nw[g][j];             // gw
                    }
                const float c1 = row_sum<G>(gy, C, lane) / (float)C;
                const float c2 = row_dot<G>(gy, z[r], C, lane) / (float)C;
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) z[r][g][j] = ((gy[g][j] - c1) - z[r][g][j] * c2) * rs;
            } else {
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) z[r][g][j] = gy[g][j];
            }
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j) sum_z[g][j] += z[r][g][j];
        }
        if (!ws_w) continue;
#pragma unroll
        for (int g = 0; g < G; ++g) {                       // dz of 256 channels -> slice as [32][256]; a thread owns a channel
            __syncthreads();
#pragma unroll
            for (int r = 0; r < kWaveRows; ++r)
                *reinterpret_cast<float4 *>(slice + (wave * kWaveRows + r) * kSpan + lane * 4) =
                    make_float4(z[r][g][0], z[r][g][1], z[r][g][2], z[r][g][3]);
            __syncthreads();
            const int c = g * kSpan + threadIdx.x;
            if (c >= C) continue;
            float col[kTile];
#pragma unroll
            for (int t = 0; t < kTile; ++t) col[t] = slice[t * kSpan + threadIdx.x];
            for (int k = 0; k < K; ++k) {
                float s = 0.0f;
#pragma unroll
                for (int t4 = 0; t4 < kTile; t4 += 4) {
                    const float4 pv = *reinterpret_cast<const float4 *>(patchT + k * kTile + t4);
                    s = fmaf(col[t4], pv.x, s);
                    s = fmaf(col[t4 + 1], pv.y, s);
                    s = fmaf(col[t4 + 2], pv.z, s);
                    s = fmaf(col[t4 + 3], pv.w, s);
                }
                float *at = ws_w + (chunk * K + k) * C + c;
                *at = tile == 0 ? s : *at + s;
            }
        }
    }
    // the chunk's column sums: the four waves ascending
    if (!ws_cols) return;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            slice[(wave * 3 + 0) * kSpan + lane * 4 + j] = sum_w[g][j];
            slice[(wave * 3 + 1) * kSpan + lane * 4 + j] = sum_b[g][j];
            slice[(wave * 3 + 2) * kSpan + lane * 4 + j] = sum_z[g][j];
        }
        __syncthreads();
        const int c = g * kSpan + threadIdx.x;
        if (c >= C) continue;
#pragma unroll
        for (int which = 0; which < 3; ++which) {
            float s = slice[which * kSpan + threadIdx.x];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) s += slice[(w * 3 + which) * kSpan + threadIdx.x];
            ws_cols[(chunk * 3 + which) * C + c] = s;
        }
    }
}

// ---- the chunks' partials -> a gradient --------------------------------------------------------------------------------------
// One wave per output element: lane l adds the chunks l, l + 64, .. ascending, butterflies, rounded once.  Element o of a job is
// (k, c) = (o / C, o % C); its partials lie at src[chunk * stride + o]; it goes to dst[c * m + k] (m = 1: a column sum).
struct Job {
    const float *src;
    void *dst;
    long long stride;
    int m;
};
struct Jobs {
    Job job[4];
};

template <typename TP>
__global__ __launch_bounds__(kThreads) void combine_kernel(const Jobs jobs, const int C, const int chunks)
{
    const Job job = jobs.job[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const long long o = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (!job.dst || o >= (long long)job.m * C) return;
    const int k = (int)(o / C), c = (int)(o - (long long)k * C);
    float s = 0.0f;
    for (int q = lane; q < chunks; q += 64) s += job.src[q * job.stride + o];
    s = wave_sum(s);
    if (lane == 0) from_acc(((TP *)job.dst)[(long long)c * job.m + k], s);
}

// ---- the output norm ---------------------------------------------------------------------------------------------------------
// where channel cl (0..255) of a group lies in the LDS tile
__device__ __forceinline__ int tile_row(int lane, int j) { return j * 64 + lane; }

// Forward: the wave's rows are normalised in registers, group after group deposited in the tile and written along the tokens.
template <typename TX, typename TY, typename TP, int G>
__global__ __launch_bounds__(kThreads) void map_forward_kernel(const TX *__restrict__ x, const TP *__restrict__ weight,
                                                               const TP *__restrict__ bias, TY *__restrict__ y,
                                                               float *__restrict__ mean_out, float *__restrict__ rstd_out,
                                                               const MGeo geo, const float eps, const int vec_)
{
    __shared__ float tile[kSpan * kPitch];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, C = geo.C;
    const bool vec = vec_ != 0;
    const long long tile0 = (long long)blockIdx.x * kTile;
    float m[kWaveRows], rs[kWaveRows];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (g > 0) __syncthreads();                         // (the last group's tile is written out)
        const int c0 = channel_of(g, lane);
        float w[4], b[4];
        load4(weight + c0, C - c0, vec, w);
        load4(bias + c0, C - c0, vec, b);
#pragma unroll
        for (int r = 0; r < kWaveRows; ++r) {
            const int t = wave * kWaveRows + r;
            const long long row = tile0 + t;
            if (row >= geo.R) break;
            float zg[4];
            if (g == 0) {                                   // the whole row: its statistics, prenorm.hip's forward
                float z[G][4];
#pragma unroll
                for (int h = 0; h < G; ++h) {
                    const int h0 = channel_of(h, lane);
                    load4(x + row * C + h0, C - h0, vec, z[h]);
                }
                const float mean = row_sum<G>(z, C, lane) / (float)C;
                float sq[G][4];
#pragma unroll
                for (int h = 0; h < G; ++h)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float d = z[h][j] - mean;
                        sq[h][j] = d * d;
                    }
                const float var = row_sum<G>(sq, C, lane) / (float)C;
                m[r] = mean;
                rs[r] = rsqrt_of(var + eps);
                if (mean_out && lane == 0) {
                    mean_out[row] = m[r];
                    rstd_out[row] = rs[r];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) zg[j] = z[0][j];
            } else {
                load4(x + row * C + c0, C - c0, vec, zg);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) tile[tile_row(lane, j) * kPitch + t] = ((zg[j] - m[r]) * rs[r]) * w[j] + b[j];
        }
        __syncthreads();
        const int t = threadIdx.x & (kTile - 1), sub = threadIdx.x / kTile;
        const long long row = tile0 + t;
        if (row < geo.R) {
            const long long b_ = row / geo.HW, hw = row - b_ * geo.HW;
            TY *base = y + b_ * C * geo.HW + hw;
            for (int i = 0; i < kSpan / (kThreads / kTile); ++i) {
                const int tr = i * (kThreads / kTile) + sub;
                const int c = g * kSpan + (tr & 63) * 4 + (tr >> 6);
                if (c < C) from_acc(base[(long long)c * geo.HW], tile[tr * kPitch + t]);
            }
        }
    }
}

// grad_y of group g of the tile's tokens -> the LDS tile, read along the tokens; 0 for a token >= R or a channel >= C
template <typename TY>
__device__ __forceinline__ void load_map_tile(const TY *__restrict__ grad_y, const MGeo &geo, long long tile0, int g, float *tile)
{
    const int t = threadIdx.x & (kTile - 1), sub = threadIdx.x / kTile;
    const long long row = tile0 + t;
    const bool live = row < geo.R;
    const long long b_ = live ? row / geo.HW : 0, hw = live ? row - b_ * geo.HW : 0;
    const TY *base = grad_y + b_ * geo.C * geo.HW + hw;
    for (int i = 0; i < kSpan / (kThreads / kTile); ++i) {
        const int tr = i * (kThreads / kTile) + sub;
        const int c = g * kSpan + (tr & 63) * 4 + (tr >> 6);
        tile[tr * kPitch + t] = live && c < geo.C ? to_acc(base[(long long)c * geo.HW]) : 0.0f;
    }
}

// Backward: workgroup `chunk` owns the rows [chunk * kTile, ...).  A first sweep over the groups gives c1 and c2 of each row
// (a lane's partial sums run over g, then j, as row_sum's do), a second one grad_x and the chunk's column sums -> ws
// [chunks][2][C].  A row of one group keeps its tile between the sweeps.
template <typename TX, typename TY, typename TP, int G>
__global__ __launch_bounds__(kThreads) void map_backward_kernel(const TX *__restrict__ x, const TP *__restrict__ weight,
                                                                const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                const TY *__restrict__ grad_y, TX *__restrict__ grad_x,
                                                                float *__restrict__ ws, const MGeo geo, const int vec_)
{
    __shared__ float tile[kSpan * kPitch];
    __shared__ float red[kWaves * 2 * kSpan];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, C = geo.C;
    const bool vec = vec_ != 0;
    const long long chunk = blockIdx.x, tile0 = chunk * kTile;
    float m[kWaveRows], rs[kWaveRows], c1[kWaveRows], c2[kWaveRows];
#pragma unroll
    for (int r = 0; r < kWaveRows; ++r) {
        const long long row = tile0 + wave * kWaveRows + r;
        m[r] = row < geo.R ? mean[row] : 0.0f;
        rs[r] = row < geo.R ? rstd[row] : 0.0f;
        c1[r] = c2[r] = 0.0f;
    }
    if (grad_x) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (g > 0) __syncthreads();
            load_map_tile(grad_y, geo, tile0, g, tile);
            __syncthreads();
            const int c0 = channel_of(g, lane);
            float w[4];
            load4(weight + c0, C - c0, vec, w);
#pragma unroll
            for (int r = 0; r < kWaveRows; ++r) {
                const int t = wave * kWaveRows + r;
                const long long row = tile0 + t;
                if (row >= geo.R) break;
                float z[4];
                load4(x + row * C + c0, C - c0, vec, z);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float xhat = (z[j] - m[r]) * rs[r];
                    const float gw = tile[tile_row(lane, j) * kPitch + t] * w[j];
                    const float p = gw * xhat;
                    c1[r] += c0 + j < C ? gw : 0.0f;
                    c2[r] += c0 + j < C ? p : 0.0f;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kWaveRows; ++r) {
            c1[r] = wave_sum(c1[r]) / (float)C;
            c2[r] = wave_sum(c2[r]) / (float)C;
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (!(G == 1 && grad_x)) {
            __syncthreads();
            load_map_tile(grad_y, geo, tile0, g, tile);
            __syncthreads();
        }
        const int c0 = channel_of(g, lane);
        float w[4], pw[4] = {0.0f, 0.0f, 0.0f, 0.0f}, pb[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (grad_x) load4(weight + c0, C - c0, vec, w);
#pragma unroll
        for (int r = 0; r < kWaveRows; ++r) {
            const int t = wave * kWaveRows + r;
            const long long row = tile0 + t;
            if (row >= geo.R) break;
            float z[4], dz[4];
            load4(x + row * C + c0, C - c0, vec, z);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xhat = (z[j] - m[r]) * rs[r];
                const float gy = tile[tile_row(lane, j) * kPitch + t];
                pw[j] += gy * xhat;
                pb[j] += gy;
                if (grad_x) {
                    const float gw = gy * w[j];
                    dz[j] = ((gw - c1[r]) - xhat * c2[r]) * rs[r];
                }
            }
            if (grad_x) store4(grad_x + row * C + c0, C - c0, vec, dz);
        }
        if (!ws) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            red[(wave * 2 + 0) * kSpan + lane * 4 + j] = pw[j];
            red[(wave * 2 + 1) * kSpan + lane * 4 + j] = pb[j];
        }
        __syncthreads();
        const int c = g * kSpan + threadIdx.x;
        if (c < C) {
#pragma unroll
            for (int which = 0; which < 2; ++which) {
                float s = red[which * kSpan + threadIdx.x];
#pragma unroll
                for (int v = 1; v < kWaves; ++v) s += red[(v * 2 + which) * kSpan + threadIdx.x];
                ws[(chunk * 2 + which) * C + c] = s;
            }
        }
        __syncthreads();                                    // (red is read before the next group writes it)
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
bool is16(int d) { return d == kBF16 || d == kF16; }
bool known(int d) { return d == kF32 || is16(d); }

int check_embed_types(const swinends_embed_types *t)
{
    if (!t) return err.fail("null pointer: types");
    if (!known(t->image) || !known(t->param) || !known(t->y))
        return err.fail("bad dtype code (float32, bfloat16 and float16 are the kernels' dtypes)");
    const bool ok = t->image == t->param && (t->y == t->image || (t->image == kF32 && is16(t->y)));
    return ok ? SWINENDS_OK : err.fail("unsupported combination of dtypes (image %lld, tokens %lld; see swinends.h)", t->image, t->y);
}

int check_map_types(const swinends_map_types *t)
{
    if (!t) return err.fail("null pointer: types");
    if (!known(t->x) || !known(t->param) || !known(t->y))
        return err.fail("bad dtype code (float32, bfloat16 and float16 are the kernels' dtypes)");
    const bool ok = t->x == kF32 ? t->param == kF32 : (t->y == t->x && (t->param == t->x || t->param == kF32));
    return ok ? SWINENDS_OK : err.fail("unsupported combination of dtypes (x %lld, y %lld; see swinends.h)", t->x, t->y);
}

int embed_geo_of(const swinends_embed_shape *s, EGeo *geo)
{
    if (!s) return err.fail("null pointer: shape");
    if (s->B < 0 || s->H < 0 || s->W < 0) return err.fail("B, H and W must not be negative");
    if (s->Cin < 1 || s->p < 1) return err.fail("Cin and p must be positive");
    if (s->C < 1) return err.fail("C must be positive, got %lld", s->C);
    if (s->C > kMaxEmbed) return err.fail("C = %lld is more than the %lld channels of the embedding kernels", s->C, kMaxEmbed);
    const long long K = (long long)s->Cin * s->p * s->p;
    if (s->p > kMaxK || K > kMaxK) return err.fail("K = Cin * p * p = %lld is more than %lld", K, kMaxK);
    if (s->B > 0x7fffffffLL) return err.fail("B = %lld does not fit 31 bits", s->B);
    geo->Cin = s->Cin, geo->H = s->H, geo->W = s->W, geo->p = s->p, geo->C = s->C, geo->K = (int)K;
    geo->Hp = (int)cdiv(s->H, s->p), geo->Wp = (int)cdiv(s->W, s->p);
    geo->HpWp = (long long)geo->Hp * geo->Wp;
    if (geo->HpWp > 0x7fffffffLL || s->B * geo->HpWp > 0x7fffffffLL) return err.fail("the tokens do not fit 31 bits");
    geo->R = s->B * geo->HpWp;
    if (geo->HpWp == 0) geo->HpWp = 1, geo->Wp = geo->Wp ? geo->Wp : 1;      // (no tokens: nothing divides by them)
    return SWINENDS_OK;
}

int map_geo_of(const swinends_map_shape *s, MGeo *geo)
{
    if (!s) return err.fail("null pointer: shape");
    if (s->B < 0 || s->H < 0 || s->W < 0) return err.fail("B, H and W must not be negative");
    if (s->C < 1) return err.fail("C must be positive, got %lld", s->C);
    if (s->C > kMaxC) return err.fail("C = %lld is more than the %lld channels a wave holds", s->C, kMaxC);
    if (s->B > 0x7fffffffLL) return err.fail("B = %lld does not fit 31 bits", s->B);
    geo->C = s->C;
    geo->HW = (long long)s->H * s->W;
    if (geo->HW > 0x7fffffffLL || s->B * geo->HW > 0x7fffffffLL) return err.fail("the rows do not fit 31 bits");
    geo->R = s->B * geo->HW;
    if (geo->HW == 0) geo->HW = 1;
    return SWINENDS_OK;
}

// f(Groups<G>) for the smallest G that covers C channels: of {1, 2, 3, 4} (the embedding), of prenorm.hip's seven (the norm)
template <typename F> int dispatch_embed_groups(int C, F &&f)
{
    const int need = (int)cdiv(C, kSpan);
    if (need <= 1) return f(Groups<1>());
    if (need <= 2) return f(Groups<2>());
    return need <= 3 ? f(Groups<3>()) : f(Groups<4>());
}

template <typename F> int dispatch_map_groups(int C, F &&f)
{
    const int need = (int)cdiv(C, kSpan);
    if (need <= 4) return dispatch_embed_groups(C, f);
    if (need <= 6) return f(Groups<6>());
    return need <= 8 ? f(Groups<8>()) : f(Groups<12>());
}

// f(Tag<TI>, Tag<TP>, Tag<TY>) of a checked combination
template <typename F> int dispatch_embed_types(const swinends_embed_types &t, F &&f)
{
    if (t.image == kBF16) return f(Tag<__hip_bfloat16>(), Tag<__hip_bfloat16>(), Tag<__hip_bfloat16>());
    if (t.image == kF16) return f(Tag<__half>(), Tag<__half>(), Tag<__half>());
    if (t.y == kBF16) return f(Tag<float>(), Tag<float>(), Tag<__hip_bfloat16>());
    if (t.y == kF16) return f(Tag<float>(), Tag<float>(), Tag<__half>());
    return f(Tag<float>(), Tag<float>(), Tag<float>());
}

// f(Tag<TX>, Tag<TY>, Tag<TP>) of a checked combination
template <typename H, typename F> int dispatch_map16(const swinends_map_types &t, F &&f)
{
    if (t.x == kF32) return f(Tag<float>(), Tag<H>(), Tag<float>());
    return t.param == kF32 ? f(Tag<H>(), Tag<H>(), Tag<float>()) : f(Tag<H>(), Tag<H>(), Tag<H>());
}

template <typename F> int dispatch_map_types(const swinends_map_types &t, F &&f)
{
    if (t.x == kF32 && t.y == kF32) return f(Tag<float>(), Tag<float>(), Tag<float>());
    return t.y == kBF16 ? dispatch_map16<__hip_bfloat16>(t, f) : dispatch_map16<__half>(t, f);
}

long long round256(long long bytes) { return (bytes + 255) / 256 * 256; }

}  // namespace swinends

using namespace swinends;

extern "C" {

int swinends_version(void) { return SWINENDS_ABI_VERSION; }

const char *swinends_last_error(void) { return err.msg; }

int swinends_tile(int which)
{
    switch (which) {
    case SWINENDS_TILE_TOKENS: return kTile;
    case SWINENDS_TILE_EMBED_CHUNK: return kEmbedChunk;
    case SWINENDS_TILE_MAX_PATCH: return kMaxK;
    case SWINENDS_TILE_MAX_EMBED: return kMaxEmbed;
    case SWINENDS_TILE_MAX_CHANNELS: return kMaxC;
    default: return -1;
    }
}

long long swinends_embed_tokens(const swinends_embed_shape *shape)
{
    err.clear();
    EGeo geo;
    if (embed_geo_of(shape, &geo) != SWINENDS_OK) return SWINENDS_ERR_ARGUMENT;
    return geo.R;
}

long long swinends_embed_workspace_bytes(const swinends_embed_shape *shape, int want_weight)
{
    err.clear();
    EGeo geo;
    if (embed_geo_of(shape, &geo) != SWINENDS_OK) return SWINENDS_ERR_ARGUMENT;
    const long long chunks = cdiv(geo.R, kEmbedChunk);
    return round256(chunks * (3 + (want_weight ? geo.K : 0)) * geo.C * (long long)sizeof(float));
}

int swinends_embed_forward(const swinends_embed_types *types, const void *image, const void *proj_weight, const void *proj_bias,
                           const void *norm_weight, const void *norm_bias, double eps, const swinends_embed_shape *shape,
                           void *tokens, float *mean, float *rstd, void *stream)
{
    err.clear();
    EGeo geo;
    if (embed_geo_of(shape, &geo) != SWINENDS_OK || check_embed_types(types) != SWINENDS_OK) return SWINENDS_ERR_ARGUMENT;
    if (!(eps == eps)) return err.fail("eps must be a number");
    if (!norm_weight != !norm_bias) return err.fail("null pointer: norm_weight and norm_bias are given together or not at all");
    if (!mean != !rstd) return err.fail("null pointer: mean and rstd are given together or not at all");
    if (mean && !norm_weight) return err.fail("mean and rstd belong to the norm, and there is none");
    if (!tokens) return err.fail("null pointer: tokens is required");
    if (geo.R == 0) return SWINENDS_OK;
    if (!image || !proj_weight) return err.fail("null pointer: image and proj_weight are required");
    const int vec = geo.C % 4 == 0 && aligned16(tokens);
    unsigned grid;
    if (err.grid_of(cdiv(geo.R, kTile), &grid) != SWINENDS_OK) return SWINENDS_ERR_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_embed_types(*types, [&](auto ti, auto tp, auto ty) {
        typedef type_of<decltype(ti)> TI;
        typedef type_of<decltype(tp)> TP;
        typedef type_of<decltype(ty)> TY;
        return dispatch_embed_groups(geo.C, [&](auto groups) {
            constexpr int G = decltype(groups)::value;
            hipLaunchKernelGGL((embed_forward_kernel<TI, TP, TY, G>), dim3(grid), dim3(kThreads), 0, st, (const TI *)image,
                               (const TP *)proj_weight, (const TP *)proj_bias, (const TP *)norm_weight, (const TP *)norm_bias,
                               (TY *)tokens, mean, rstd, geo, (float)eps, vec);
            return err.check_launch("swinends_embed_forward");
        });
    });
}

int swinends_embed_backward(const swinends_embed_types *types, const void *image, const void *proj_weight, const void *proj_bias,
                            const void *norm_weight, const float *mean, const float *rstd, const void *grad_tokens,
                            const swinends_embed_shape *shape, void *workspace, void *grad_proj_weight, void *grad_proj_bias,
                            void *grad_norm_weight, void *grad_norm_bias, void *stream)
{
    err.clear();
    EGeo geo;
    if (embed_geo_of(shape, &geo) != SWINENDS_OK || check_embed_types(types) != SWINENDS_OK) return SWINENDS_ERR_ARGUMENT;
    if (!grad_proj_weight && !grad_proj_bias && !grad_norm_weight && !grad_norm_bias) return err.fail("no gradient is asked for");
    if (!norm_weight != !mean || !mean != !rstd)
        return err.fail("null pointer: norm_weight, mean and rstd are given together or not at all");
    if (!norm_weight && (grad_norm_weight || grad_norm_bias)) return err.fail("grad_norm_weight and grad_norm_bias belong to the norm, and there is none");
    if (geo.R == 0) return err.fail("no tokens: the gradients are zero and this call writes nothing");
    if (!image || !proj_weight || !grad_tokens) return err.fail("null pointer: image, proj_weight and grad_tokens are required");
    if (!workspace) return err.fail("null pointer: workspace is required");
    if (!aligned16(workspace)) return err.fail("the workspace must be 16-byte aligned");
    const long long chunks = cdiv(geo.R, kEmbedChunk);
    float *ws_cols = (float *)workspace, *ws_w = grad_proj_weight ? ws_cols + chunks * 3 * geo.C : nullptr;
    const int vec = geo.C % 4 == 0 && aligned16(grad_tokens);
    const long long most = grad_proj_weight ? (long long)geo.K * geo.C : geo.C;
    Jobs jobs;
    jobs.job[0] = {ws_cols, grad_norm_weight, 3LL * geo.C, 1};
    jobs.job[1] = {ws_cols + geo.C, grad_norm_bias, 3LL * geo.C, 1};
    jobs.job[2] = {ws_cols + 2 * geo.C, grad_proj_bias, 3LL * geo.C, 1};
    jobs.job[3] = {ws_w, grad_proj_weight, (long long)geo.K * geo.C, geo.K};
    hipStream_t st = (hipStream_t)stream;
    return dispatch_embed_types(*types, [&](auto ti, auto tp, auto ty) {
        typedef type_of<decltype(ti)> TI;
        typedef type_of<decltype(tp)> TP;
        typedef type_of<decltype(ty)> TY;
        return dispatch_embed_groups(geo.C, [&](auto groups) {
            constexpr int G = decltype(groups)::value;
            hipLaunchKernelGGL((embed_backward_kernel<TI, TP, TY, G>), dim3((unsigned)chunks), dim3(kThreads), 0, st,
                               (const TI *)image, (const TP *)proj_weight, (const TP *)proj_bias, (const TP *)norm_weight, mean, rstd,
                               (const TY *)grad_tokens, ws_cols, ws_w, geo, vec);
            hipLaunchKernelGGL((combine_kernel<TP>), dim3((unsigned)cdiv(most, kWaves), 4), dim3(kThreads), 0, st, jobs, geo.C,
                               (int)chunks);
            return err.check_launch("swinends_embed_backward");
        });
    });
}

long long swinends_map_workspace_bytes(const swinends_map_shape *shape)
{
    err.clear();
    MGeo geo;
    if (map_geo_of(shape, &geo) != SWINENDS_OK) return SWINENDS_ERR_ARGUMENT;
    return round256(cdiv(geo.R, kTile) * 2 * geo.C * (long long)sizeof(float));
}

int swinends_map_forward(const swinends_map_types *types, const void *x, const void *weight, const void *bias, double eps,
                         const swinends_map_shape *shape, void *y, float *mean, float *rstd, void *stream)
{
    err.clear();
    MGeo geo;
    if (map_geo_of(shape, &geo) != SWINENDS_OK || check_map_types(types) != SWINENDS_OK) return SWINENDS_ERR_ARGUMENT;
    if (!(eps == eps)) return err.fail("eps must be a number");
    if (!y) return err.fail("null pointer: y is required");
    if (!mean != !rstd) return err.fail("null pointer: mean and rstd are given together or not at all");
    if (geo.R == 0) return SWINENDS_OK;
    if (!x || !weight || !bias) return err.fail("null pointer: x, weight and bias are required");
    const int vec = geo.C % 4 == 0 && aligned16(x) && aligned16(weight) && aligned16(bias);
    unsigned grid;
    if (err.grid_of(cdiv(geo.R, kTile), &grid) != SWINENDS_OK) return SWINENDS_ERR_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_map_types(*types, [&](auto tx, auto ty, auto tp) {
        typedef type_of<decltype(tx)> TX;
        typedef type_of<decltype(ty)> TY;
        typedef type_of<decltype(tp)> TP;
        return dispatch_map_groups(geo.C, [&](auto groups) {
            constexpr int G = decltype(groups)::value;
            hipLaunchKernelGGL((map_forward_kernel<TX, TY, TP, G>), dim3(grid), dim3(kThreads), 0, st, (const TX *)x,
                               (const TP *)weight, (const TP *)bias, (TY *)y, mean, rstd, geo, (float)eps, vec);
            return err.check_launch("swinends_map_forward");
        });
    });
}

int swinends_map_backward(const swinends_map_types *types, const void *x, const void *weight, const float *mean, const float *rstd,
                          const void *grad_y, const swinends_map_shape *shape, void *workspace, void *grad_x, void *grad_weight,
                          void *grad_bias, void *stream)
{
    err.clear();
    MGeo geo;
    if (map_geo_of(shape, &geo) != SWINENDS_OK || check_map_types(types) != SWINENDS_OK) return SWINENDS_ERR_ARGUMENT;
    if (!grad_x && !grad_weight && !grad_bias) return err.fail("no gradient is asked for");
    if (geo.R == 0) return err.fail("no rows: the gradients are zero and this call writes nothing");
    if (!x || !mean || !rstd || !grad_y) return err.fail("null pointer: x, mean, rstd and grad_y are required");
    if (grad_x && !weight) return err.fail("null pointer: weight is required for grad_x");
    const bool params = grad_weight || grad_bias;
    if (params && !workspace) return err.fail("null pointer: workspace is required for grad_weight and grad_bias");
    if (!aligned16(workspace)) return err.fail("the workspace must be 16-byte aligned");
    const int vec = geo.C % 4 == 0 && aligned16(x) && aligned16(weight) && aligned16(grad_x);
    unsigned grid;
    if (err.grid_of(cdiv(geo.R, kTile), &grid) != SWINENDS_OK) return SWINENDS_ERR_ARGUMENT;
    float *ws = params ? (float *)workspace : nullptr;
    Jobs jobs = {};
    jobs.job[0] = {ws, grad_weight, 2LL * geo.C, 1};
    jobs.job[1] = {ws ? ws + geo.C : nullptr, grad_bias, 2LL * geo.C, 1};
    hipStream_t st = (hipStream_t)stream;
    return dispatch_map_types(*types, [&](auto tx, auto ty, auto tp) {
        typedef type_of<decltype(tx)> TX;
        typedef type_of<decltype(ty)> TY;
        typedef type_of<decltype(tp)> TP;
        return dispatch_map_groups(geo.C, [&](auto groups) {
            constexpr int G = decltype(groups)::value;
            hipLaunchKernelGGL((map_backward_kernel<TX, TY, TP, G>), dim3(grid), dim3(kThreads), 0, st, (const TX *)x,
                               (const TP *)weight, mean, rstd, (const TY *)grad_y, (TX *)grad_x, ws, geo, vec);
            if (params)
                hipLaunchKernelGGL((combine_kernel<TP>), dim3((unsigned)cdiv(geo.C, kWaves), 2), dim3(kThreads), 0, st, jobs, geo.C,
                                   (int)grid);
            return err.check_launch("swinends_map_backward");
        });
    });
}

}  // extern "C"
