// prenorm.hip -- the glue of the Swin backbone's blocks (include/prenorm.h): the residual add with its
// drop-path scale, the pre-norm LayerNorm, the store into the zero-padded window map and the 2 x 2 patch gather, forward and
// backward, each one pass.  gfx950, wave64, plain HIP.  addnorm.hip's design at up to 3072 channels: one wave owns a row and
// holds it in registers; there is no LDS, no atomic and nothing is zeroed by a pass of its own.  The row itself -- a lane's
// quads and the sums over the channels -- is norm_row.h's (devis::normrow, a part of op_common.h), which swinends.hip shares.
#include "op_common.h"       // (fp contraction off)
#include "prenorm.h"

namespace prenorm {

using namespace devis;
using namespace devis::normrow;

static_assert(PRENORM_OK == kOk && PRENORM_ERR_ARGUMENT == kErrArgument && PRENORM_ERR_HIP == kErrHip, "status codes");
static_assert(PRENORM_F32 == kF32 && PRENORM_BF16 == kBF16 && PRENORM_F16 == kF16, "dtype codes");

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxC = PRENORM_MAX_CHANNELS;
constexpr int kChunkRows = 32;              // rows of one chunk of the backward's column sums

thread_local Status err;     // prenorm_last_error()

// what the kernels know of a call (host: geo_of)
struct Geo {
    long long R;            // rows
    long long slots;        // waves of the forward: R, or the positions of the map
    long long HW;           // H * W
    int H, W, C, Cin;       // Cin: x's channels (C / 4 in MERGE, C otherwise)
    int Hp, Wp;             // the map (dest == MAP)
    int H2, W2;             // the merged map (source == MERGE)
    int source, dest;
};

// ---- the 2 x 2 gather -----------------------------------------------------------------------------------------------------
// the merged row's position
struct Cell {
    long long b;
    int i, j;
};

__device__ __forceinline__ Cell cell_of(const Geo &geo, long long row)
{
    Cell c;
    const long long t = row / geo.W2;
    c.j = (int)(row - t * geo.W2);
    c.b = t / geo.H2;
    c.i = (int)(t - c.b * geo.H2);
    return c;
}

// element offset in x [B, H, W, Cin] of channel c < C of the merged row at `cell`, or -1 where the piece is padding
__device__ __forceinline__ long long merge_offset(const Geo &geo, const Cell &cell, int c)
{
    const int q = (c >= geo.Cin) + (c >= 2 * geo.Cin) + (c >= 3 * geo.Cin);
    const int h = 2 * cell.i + (q & 1), w = 2 * cell.j + (q >> 1);
    if (h >= geo.H || w >= geo.W) return -1;
    return ((cell.b * geo.H + h) * geo.W + w) * geo.Cin + (c - q * geo.Cin);
}

// ---- a row ------------------------------------------------------------------------------------------------------------------
// A(x) of row `row`, channels >= C as 0: dense, or gathered in MERGE
template <typename TX, int G>
__device__ __forceinline__ void gather_row(const TX *__restrict__ x, const Geo &geo, long long row, int lane, bool vec,
                                           float (&z)[G][4])
{
    const int C = geo.C;
    if (geo.source != PRENORM_MERGE) {
        const TX *p = x + row * C;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int c0 = channel_of(g, lane);
            load4(p + c0, C - c0, vec, z[g]);
        }
        return;
    }
    const Cell cell = cell_of(geo, row);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c0 = channel_of(g, lane);
        if (vec) {                                          // (Cin % 4 == 0: a quad lies in one piece)
            const long long at = c0 < C ? merge_offset(geo, cell, c0) : -1;
            load4(x + (at < 0 ? 0 : at), at < 0 ? 0 : 4, true, z[g]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long at = c0 + j < C ? merge_offset(geo, cell, c0 + j) : -1;
                z[g][j] = at < 0 ? 0.0f : to_acc(x[at]);
            }
        }
    }
}

// dz of a row -> grad_x: dense, or scattered to the gathered positions in MERGE (a padded piece is dropped)
template <typename TX>
__device__ __forceinline__ void scatter4(TX *__restrict__ grad_x, const Geo &geo, long long row, const Cell &cell, int c0, bool vec,
                                         const float (&dz)[4])
{
    const int C = geo.C;
    if (geo.source != PRENORM_MERGE) {
        store4(grad_x + row * C + c0, C - c0, vec, dz);
    } else if (vec) {
        const long long at = c0 < C ? merge_offset(geo, cell, c0) : -1;
        if (at >= 0) store4(grad_x + at, 4, true, dz);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long at = c0 + j < C ? merge_offset(geo, cell, c0 + j) : -1;
            if (at >= 0) from_acc(grad_x[at], dz[j]);
        }
    }
}

// the element offset of row `row`'s y (and grad_y)
__device__ __forceinline__ long long dest_offset(const Geo &geo, long long row)
{
    if (geo.dest != PRENORM_MAP) return row * geo.C;
    const long long b = row / geo.HW, t = row - b * geo.HW;
    const long long h = t / geo.W, w = t - h * geo.W;
    return ((b * geo.Hp + h) * geo.Wp + w) * geo.C;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
// One wave per slot: a row, or with a map one position of it -- a token's row, or padding, written as 0.
template <typename TX, typename TD, typename TY, typename TP, int G>
__global__ __launch_bounds__(kThreads) void forward_kernel(const TX *__restrict__ x, const TD *__restrict__ delta,
                                                           const float *__restrict__ keep, const TP *__restrict__ weight,
                                                           const TP *__restrict__ bias, TX *__restrict__ s, TY *__restrict__ y,
                                                           float *__restrict__ mean_out, float *__restrict__ rstd_out,
                                                           const Geo geo, const float eps, const int vec_)
{
    const int lane = threadIdx.x & 63, C = geo.C;
    const bool vec = vec_ != 0;
    const long long slot = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (slot >= geo.slots) return;
    long long row = slot, yoff = slot * C;
    if (geo.dest == PRENORM_MAP) {
        const long long t = slot / geo.Wp, b = t / geo.Hp;
        const int w = (int)(slot - t * geo.Wp), h = (int)(t - b * geo.Hp);
        if (h >= geo.H || w >= geo.W) {
            const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int c0 = channel_of(g, lane);
                store4(y + yoff + c0, C - c0, vec, zero);
            }
            return;
        }
        row = (b * geo.H + h) * geo.W + w;
    }
    float z[G][4];
    gather_row<TX, G>(x, geo, row, lane, vec, z);
    if (geo.source == PRENORM_RESIDUAL) {
        const float k = keep ? keep[row / geo.HW] : 1.0f;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int c0 = channel_of(g, lane);
            if (k != 0.0f) {
                float d[4];
                load4(delta + row * C + c0, C - c0, vec, d);
#pragma unroll
                for (int j = 0; j < 4; ++j) z[g][j] = rounded<TX>(z[g][j] + d[j] * k);
            }
            store4(s + row * C + c0, C - c0, vec, z[g]);
        }
    }
    const float mean = row_sum<G>(z, C, lane) / (float)C;
    float sq[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float t = z[g][j] - mean;
            sq[g][j] = t * t;
        }
    const float var = row_sum<G>(sq, C, lane) / (float)C;
    const float rstd = rsqrt_of(var + eps);
    if (mean_out && lane == 0) {
        mean_out[row] = mean;
        rstd_out[row] = rstd;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c0 = channel_of(g, lane);
        float w[4], b[4], out[4];
        load4(weight + c0, C - c0, vec, w);
        load4(bias + c0, C - c0, vec, b);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = ((z[g][j] - mean) * rstd) * w[j] + b[j];
        store4(y + yoff + c0, C - c0, vec, out);
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// Wave `chunk` owns the rows [chunk * kChunkRows, ...): grad_x and grad_delta of each, and the column partials of g * xhat and
// g, rows ascending, -> ws[(chunk * 2 + which) * C + c], or the results themselves when the call is one chunk.  The weight is
// read again for every row (from the cache) instead of being held: at 12 groups the row, its gradient and the two partials are
// 192 registers of a lane already.
template <typename TX, typename TD, typename TY, typename TP, int G>
__global__ __launch_bounds__(kThreads) void backward_kernel(const TX *__restrict__ x, const float *__restrict__ keep,
                                                            const TP *__restrict__ weight, const float *__restrict__ mean,
                                                            const float *__restrict__ rstd, const TY *__restrict__ grad_y,
                                                            const TX *__restrict__ grad_s, TX *__restrict__ grad_x,
                                                            TD *__restrict__ grad_delta, float *__restrict__ ws,
                                                            TP *__restrict__ grad_weight, TP *__restrict__ grad_bias,
                                                            const Geo geo, const int chunks, const int vec_)
{
    const int lane = threadIdx.x & 63, C = geo.C;
    const bool vec = vec_ != 0;
    const long long chunk = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (chunk >= chunks) return;
    const bool want_dz = grad_x || grad_delta, want_params = grad_weight || grad_bias;
    const long long row0 = chunk * kChunkRows;
    const long long row1 = geo.R - row0 < kChunkRows ? geo.R : row0 + kChunkRows;
    float pw[G][4], pb[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) pw[g][j] = pb[g][j] = 0.0f;
    for (long long row = row0; row < row1; ++row) {
        float z[G][4], gy[G][4];
        gather_row<TX, G>(x, geo, row, lane, vec, z);
        const float m = mean[row], rs = rstd[row];
        const long long yoff = dest_offset(geo, row);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int c0 = channel_of(g, lane);
            load4(grad_y + yoff + c0, C - c0, vec, gy[g]);
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
        if (!want_dz) continue;
#pragma unroll
        for (int g = 0; g < G; ++g) {                                           // gy becomes gw = g * weight
            const int c0 = channel_of(g, lane);
            float w[4];
            load4(weight + c0, C - c0, vec, w);
#pragma unroll
            for (int j = 0; j < 4; ++j) gy[g][j] = gy[g][j] * w[j];
        }
        const float c1 = row_sum<G>(gy, C, lane) / (float)C;
        const float c2 = row_dot<G>(gy, z, C, lane) / (float)C;
        const float k = keep ? keep[row / geo.HW] : 1.0f;
        Cell cell = {0, 0, 0};
        if (geo.source == PRENORM_MERGE) cell = cell_of(geo, row);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int c0 = channel_of(g, lane);
            float dz[4], dd[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) dz[j] = ((gy[g][j] - c1) - z[g][j] * c2) * rs;
            if (grad_s) {
                float gs[4];
                load4(grad_s + row * C + c0, C - c0, vec, gs);
#pragma unroll
                for (int j = 0; j < 4; ++j) dz[j] = dz[j] + gs[j];
            }
            if (grad_x) scatter4(grad_x, geo, row, cell, c0, vec, dz);
            if (grad_delta) {
#pragma unroll
                for (int j = 0; j < 4; ++j) dd[j] = k != 0.0f ? dz[j] * k : 0.0f;
                store4(grad_delta + row * C + c0, C - c0, vec, dd);
            }
        }
    }
    if (!want_params) return;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c0 = channel_of(g, lane);
        if (chunks == 1) {
            if (grad_weight) store4(grad_weight + c0, C - c0, vec, pw[g]);
            if (grad_bias) store4(grad_bias + c0, C - c0, vec, pb[g]);
        } else {                                            // (the workspace is 16-byte aligned and C % 4 == 0 when vec)
            store4(ws + (chunk * 2 + 0) * C + c0, C - c0, vec, pw[g]);
            store4(ws + (chunk * 2 + 1) * C + c0, C - c0, vec, pb[g]);
        }
    }
}

// One wave per column and sum: lane l adds the chunks l, l + 64, .. ascending, butterflies, rounded once.
template <typename TP>
__global__ __launch_bounds__(kThreads) void combine_kernel(const float *__restrict__ ws, TP *__restrict__ grad_weight,
                                                           TP *__restrict__ grad_bias, const int C, const int chunks)
{
    const int lane = threadIdx.x & 63, c = blockIdx.x * kWaves + (threadIdx.x >> 6), which = blockIdx.y;
    TP *dst = which ? grad_bias : grad_weight;
    if (c >= C || !dst) return;
    const float *src = ws + (long long)which * C + c;
    float s = 0.0f;
    for (int k = lane; k < chunks; k += 64) s += src[(long long)k * 2 * C];
    s = wave_sum(s);
    if (lane == 0) from_acc(dst[c], s);
}

// ---- host -------------------------------------------------------------------------------------------------------------------
bool is16(int d) { return d == kBF16 || d == kF16; }
bool known(int d) { return d == kF32 || is16(d); }

int check_types(const prenorm_types *t, int source)
{
    if (!t) return err.fail("null pointer: types");
    if (!known(t->x) || !known(t->delta) || !known(t->y) || !known(t->param))
        return err.fail("bad dtype code (float32, bfloat16 and float16 are the kernels' dtypes)");
    if (source != PRENORM_RESIDUAL && t->delta != t->x) return err.fail("without a delta, types.delta must equal types.x");
    bool ok;
    if (t->x == kF32) {
        const bool narrow = (t->delta == kF32 || t->y == kF32 || t->delta == t->y);        // (at most one 16-bit dtype)
        ok = t->param == kF32 && narrow;
    } else {
        ok = t->delta == t->x && t->y == t->x && (t->param == t->x || t->param == kF32);
    }
    return ok ? PRENORM_OK : err.fail("unsupported combination of dtypes (x %lld, delta %lld; see prenorm.h)", t->x, t->delta);
}

int geo_of(const prenorm_shape *s, Geo *geo)
{
    if (!s) return err.fail("null pointer: shape");
    if (s->source != PRENORM_PLAIN && s->source != PRENORM_RESIDUAL && s->source != PRENORM_MERGE)
        return err.fail("bad source form %lld", s->source);
    if (s->dest != PRENORM_TOKENS && s->dest != PRENORM_MAP) return err.fail("bad destination form %lld", s->dest);
    if (s->B < 0 || s->H < 0 || s->W < 0) return err.fail("B, H and W must not be negative");
    if (s->C < 1) return err.fail("C must be positive, got %lld", s->C);
    if (s->C > kMaxC) return err.fail("C = %lld is more than the %lld channels a wave holds", s->C, kMaxC);
    const bool merge = s->source == PRENORM_MERGE, map = s->dest == PRENORM_MAP;
    if (merge && s->C % 4) return err.fail("a merged row has four pieces: C = %lld is not a multiple of 4", s->C);
    if (merge && map) return err.fail("a merged row has no map destination");
    if (map && (s->Hp < s->H || s->Wp < s->W)) return err.fail("the map (%lld x %lld) is smaller than the tokens' H x W", s->Hp, s->Wp);
    if (s->B > 0x7fffffffLL) return err.fail("B = %lld does not fit 31 bits", s->B);
    geo->H = s->H, geo->W = s->W, geo->C = s->C, geo->Cin = merge ? s->C / 4 : s->C;
    geo->Hp = map ? s->Hp : 0, geo->Wp = map ? s->Wp : 0;
    geo->H2 = (s->H + 1) / 2, geo->W2 = (s->W + 1) / 2;
    geo->source = s->source, geo->dest = s->dest;
    geo->HW = (long long)s->H * s->W;
    const long long per = merge ? (long long)geo->H2 * geo->W2 : geo->HW;
    const long long positions = map ? (long long)s->Hp * s->Wp : per;
    if (per > 0x7fffffffLL || positions > 0x7fffffffLL || s->B * per > 0x7fffffffLL || s->B * positions > 0x7fffffffLL)
        return err.fail("the rows do not fit 31 bits");
    geo->R = s->B * per;
    geo->slots = s->B * positions;
    if (geo->HW == 0) geo->HW = 1;                           // (no rows: nothing divides by it)
    if (geo->W2 == 0) geo->W2 = 1;
    if (geo->H2 == 0) geo->H2 = 1;
    return PRENORM_OK;
}

// f(Groups<G>) for the smallest G of {1, 2, 3, 4, 6, 8, 12} that covers C channels
template <typename F> int dispatch_groups(int C, F &&f)
{
    const int need = (int)cdiv(C, kSpan);
    if (need <= 1) return f(Groups<1>());
    if (need <= 2) return f(Groups<2>());
    if (need <= 3) return f(Groups<3>());
    if (need <= 4) return f(Groups<4>());
    if (need <= 6) return f(Groups<6>());
    return need <= 8 ? f(Groups<8>()) : f(Groups<12>());
}

// f(Tag<TX>, Tag<TD>, Tag<TY>, Tag<TP>) of a checked combination
template <typename H, typename F> int dispatch16(const prenorm_types &t, F &&f)
{
    if (t.x != kF32) return t.param == kF32 ? f(Tag<H>(), Tag<H>(), Tag<H>(), Tag<float>()) : f(Tag<H>(), Tag<H>(), Tag<H>(), Tag<H>());
    if (t.delta != kF32) return t.y != kF32 ? f(Tag<float>(), Tag<H>(), Tag<H>(), Tag<float>()) : f(Tag<float>(), Tag<H>(), Tag<float>(), Tag<float>());
    return f(Tag<float>(), Tag<float>(), Tag<H>(), Tag<float>());
}

template <typename F> int dispatch_types(const prenorm_types &t, F &&f)
{
    if (t.x == kF32 && t.delta == kF32 && t.y == kF32) return f(Tag<float>(), Tag<float>(), Tag<float>(), Tag<float>());
    const int half = t.x != kF32 ? t.x : (t.delta != kF32 ? t.delta : t.y);
    return half == kBF16 ? dispatch16<__hip_bfloat16>(t, f) : dispatch16<__half>(t, f);
}

int chunks_of(const Geo &geo) { return (int)cdiv(geo.R, kChunkRows); }

}  // namespace prenorm

using namespace prenorm;

extern "C" {

int prenorm_version(void) { return PRENORM_ABI_VERSION; }

const char *prenorm_last_error(void) { return err.msg; }

int prenorm_tile(int which)
{
    switch (which) {
    case PRENORM_TILE_ROWS: return kChunkRows;
    case PRENORM_TILE_CHANNELS: return kMaxC;
    default: return -1;
    }
}

long long prenorm_rows(const prenorm_shape *shape)
{
    err.clear();
    Geo geo;
    if (geo_of(shape, &geo) != PRENORM_OK) return PRENORM_ERR_ARGUMENT;
    return geo.R;
}

long long prenorm_workspace_bytes(const prenorm_shape *shape)
{
    err.clear();
    Geo geo;
    if (geo_of(shape, &geo) != PRENORM_OK) return PRENORM_ERR_ARGUMENT;
    const int chunks = chunks_of(geo);
    const long long bytes = chunks > 1 ? (long long)chunks * 2 * geo.C * (long long)sizeof(float) : 0;
    return (bytes + 255) / 256 * 256;
}

int prenorm_forward(const prenorm_types *types, const void *x, const void *delta, const float *keep, const void *weight,
                    const void *bias, double eps, const prenorm_shape *shape, void *s, void *y, float *mean, float *rstd,
                    void *stream)
{
    err.clear();
    Geo geo;
    if (geo_of(shape, &geo) != PRENORM_OK || check_types(types, shape->source) != PRENORM_OK) return PRENORM_ERR_ARGUMENT;
    if (!(eps == eps)) return err.fail("eps must be a number");
    const bool residual = geo.source == PRENORM_RESIDUAL;
    if (!residual && (delta || s || keep)) return err.fail("delta, s and keep belong to the residual form");
    if (!y) return err.fail("null pointer: y is required");
    if (!mean != !rstd) return err.fail("null pointer: mean and rstd are given together or not at all");
    if (geo.slots == 0) return PRENORM_OK;
    if (geo.R > 0 && (!x || !weight || !bias)) return err.fail("null pointer: x, weight and bias are required");
    if (geo.R > 0 && residual && (!delta || !s)) return err.fail("null pointer: delta and s are required in the residual form");
    const int vec = geo.Cin % 4 == 0 && aligned16(x) && aligned16(delta) && aligned16(weight) && aligned16(bias) &&
                    aligned16(s) && aligned16(y);
    unsigned grid;
    if (err.grid_of(cdiv(geo.slots, kWaves), &grid) != PRENORM_OK) return PRENORM_ERR_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_types(*types, [&](auto tx, auto td, auto ty, auto tp) {
        typedef type_of<decltype(tx)> TX;
        typedef type_of<decltype(td)> TD;
        typedef type_of<decltype(ty)> TY;
        typedef type_of<decltype(tp)> TP;
        return dispatch_groups(geo.C, [&](auto groups) {
            constexpr int G = decltype(groups)::value;
            hipLaunchKernelGGL((forward_kernel<TX, TD, TY, TP, G>), dim3(grid), dim3(kThreads), 0, st, (const TX *)x,
                               (const TD *)delta, keep, (const TP *)weight, (const TP *)bias, (TX *)s, (TY *)y, mean, rstd, geo,
                               (float)eps, vec);
            return err.check_launch("prenorm_forward");
        });
    });
}

int prenorm_backward(const prenorm_types *types, const void *x, const float *keep, const void *weight, const float *mean,
                     const float *rstd, const void *grad_y, const void *grad_s, const prenorm_shape *shape, void *workspace,
                     void *grad_x, void *grad_delta, void *grad_weight, void *grad_bias, void *stream)
{
    err.clear();
    Geo geo;
    if (geo_of(shape, &geo) != PRENORM_OK || check_types(types, shape->source) != PRENORM_OK) return PRENORM_ERR_ARGUMENT;
    if (!grad_x && !grad_delta && !grad_weight && !grad_bias) return err.fail("no gradient is asked for");
    if (geo.source != PRENORM_RESIDUAL && (grad_delta || grad_s || keep))
        return err.fail("grad_delta, grad_s and keep belong to the residual form");
    if (geo.R == 0) return PRENORM_OK;
    if (!x || !mean || !rstd || !grad_y) return err.fail("null pointer: x, mean, rstd and grad_y are required");
    if ((grad_x || grad_delta) && !weight) return err.fail("null pointer: weight is required for grad_x and grad_delta");
    const int chunks = chunks_of(geo);
    const bool params = grad_weight || grad_bias;
    if (params && chunks > 1 && !workspace) return err.fail("null pointer: workspace is required when the column sums span chunks");
    if (!aligned16(workspace)) return err.fail("the workspace must be 16-byte aligned");
    const int vec = geo.Cin % 4 == 0 && aligned16(x) && aligned16(weight) && aligned16(grad_y) && aligned16(grad_s) &&
                    aligned16(grad_x) && aligned16(grad_delta) && aligned16(grad_weight) && aligned16(grad_bias);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_types(*types, [&](auto tx, auto td, auto ty, auto tp) {
        typedef type_of<decltype(tx)> TX;
        typedef type_of<decltype(td)> TD;
        typedef type_of<decltype(ty)> TY;
        typedef type_of<decltype(tp)> TP;
        return dispatch_groups(geo.C, [&](auto groups) {
            constexpr int G = decltype(groups)::value;
            hipLaunchKernelGGL((backward_kernel<TX, TD, TY, TP, G>), dim3((unsigned)cdiv(chunks, kWaves)), dim3(kThreads), 0, st,
                               (const TX *)x, keep, (const TP *)weight, mean, rstd, (const TY *)grad_y, (const TX *)grad_s,
                               (TX *)grad_x, (TD *)grad_delta, (float *)workspace, (TP *)grad_weight, (TP *)grad_bias, geo,
                               chunks, vec);
            if (params && chunks > 1)
                hipLaunchKernelGGL((combine_kernel<TP>), dim3((unsigned)cdiv(geo.C, kWaves), 2), dim3(kThreads), 0, st,
                                   (const float *)workspace, (TP *)grad_weight, (TP *)grad_bias, geo.C, chunks);
            return err.check_launch("prenorm_backward");
        });
    });
}

}  // extern "C"
