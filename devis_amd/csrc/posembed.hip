// posembed.hip -- the encoder's positional input (include/posembed.h): the counts behind the sine
// embedding, the flattened masks and the valid ratios from the padding masks in one launch; the embedding of every token plus
// the temporal and the level embedding written once, channels last at the level's token offset (or as [N, C, H, W] for one
// level); and the gradient of the two embeddings as a segmented column sum without atomics.  gfx950, wave64, plain HIP.
#include "op_common.h"       // (fp contraction off)
#include "posembed.h"

namespace posembed {

using namespace devis;

static_assert(POSEMBED_OK == kOk && POSEMBED_ERR_ARGUMENT == kErrArgument && POSEMBED_ERR_HIP == kErrHip, "status codes");
static_assert(POSEMBED_F32 == kF32 && POSEMBED_F64 == kF64 && POSEMBED_BF16 == kBF16 && POSEMBED_F16 == kF16, "dtype codes");

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxLevels = POSEMBED_MAX_LEVELS;
constexpr int kChunkTokens = 256;           // tokens of one level and frame per workgroup of the partial pass
constexpr int kChunkChannels = 64;          // channels per workgroup of the partial pass: one per lane of a wave

thread_local Status err;     // posembed_last_error()

// What the kernels need of a shape, made on the host (geometry_of): token, column and row offsets of every level and the
// regions of the counts workspace.
struct Geo {
    int N, L, C, S, SW, SH;                             // S tokens, SW columns, SH rows per frame over all levels
    int H[kMaxLevels], W[kMaxLevels];
    int start[kMaxLevels], xoff[kMaxLevels], yoff[kMaxLevels];
    long long off_cx, off_ty, off_tx, counts_bytes;     // byte offsets of cx, ty, tx in the workspace (cy is at 0)
};

// The workgroups of the counts pass, per frame: level 0's row groups, its column groups, level 1's, ...
struct CountJobs {
    int rows[kMaxLevels], cols[kMaxLevels], per_frame;
};

// The chunks of the backward's partial pass, per frame: level l owns [first[l], first[l] + count[l]); `order`: the levels
// in the order grad_temporal_embed adds them.
struct Chunks {
    int first[kMaxLevels], count[kMaxLevels], order[kMaxLevels], per_frame;
};

// ---- counts --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void counts_kernel(const posembed_masks m, const Geo g, const CountJobs jobs,
                                                          int *__restrict__ cy, int *__restrict__ cx, int *__restrict__ ty,
                                                          int *__restrict__ tx, unsigned char *__restrict__ mask_flatten,
                                                          float *__restrict__ valid_ratios)
{
    const int n = blockIdx.x / jobs.per_frame, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int r = blockIdx.x % jobs.per_frame, l = 0;
    bool row_job = true;
    for (; l < g.L; ++l) {                  // (the same in every lane)
        if (r < jobs.rows[l]) break;
        r -= jobs.rows[l];
        if (r < jobs.cols[l]) {
            row_job = false;
            break;
        }
        r -= jobs.cols[l];
    }
    if (l >= g.L) return;
    const int H = g.H[l], W = g.W[l];
    const long long base = (long long)n * g.S + g.start[l];
    const unsigned char *frame = m.ptr[l] + (long long)n * m.sn[l];
    if (row_job) {
        // one wave per row: ballots over 64-pixel chunks, the count carried from chunk to chunk
        const int y = r * kWaves + wave;
        if (y >= H) return;
        const unsigned char *row = frame + (long long)y * m.sy[l];
        const long long out = base + (long long)y * W;
        const unsigned long long below = (2ull << lane) - 1ull;        // lanes 0..lane (all ones for lane 63)
        int carry = 0;
        for (int x0 = 0; x0 < W; x0 += 64) {
            const int x = x0 + lane;
            const bool in = x < W;
            const unsigned char byte = in ? row[(long long)x * m.sx[l]] : (unsigned char)1;
            const unsigned long long open = __ballot(in && byte == 0);
            if (in) {
                cx[out + x] = carry + __popcll(open & below);
                if (mask_flatten) mask_flatten[out + x] = byte != 0 ? 1 : 0;
            }
            carry += __popcll(open);
        }
        if (lane == 0) {
            tx[(long long)n * g.SH + g.yoff[l] + y] = carry;
            if (y == 0 && valid_ratios) valid_ratios[((long long)n * g.L + l) * 2 + 0] = (float)carry * (1.0f / (float)W);
        }
    } else {
        // one lane per column, walking down the rows
        const int x = r * kThreads + tid;
        if (x >= W) return;
        const unsigned char *col = frame + (long long)x * m.sx[l];
        int acc = 0;
        for (int y = 0; y < H; ++y) {
            acc += col[(long long)y * m.sy[l]] == 0 ? 1 : 0;
            cy[base + (long long)y * W + x] = acc;
        }
        ty[(long long)n * g.SW + g.xoff[l] + x] = acc;
        if (x == 0 && valid_ratios) valid_ratios[((long long)n * g.L + l) * 2 + 1] = (float)acc * (1.0f / (float)H);
    }
}

// ---- write ---------------------------------------------------------------------------------------------------------------
struct Coord {
    float ey, ex;
    int n, l;
};

// The two coordinates of token `tok` in [0, N * S), with the reference's float32 operations in the reference's order.
__device__ __forceinline__ Coord coord_of(const Geo &g, const int tok, const int *__restrict__ cy, const int *__restrict__ cx,
                                          const int *__restrict__ ty, const int *__restrict__ tx, const int normalize,
                                          const float scale)
{
    Coord q;
    q.n = tok / g.S;
    const int s = tok - q.n * g.S;
    int l = g.L - 1;
    while (l > 0 && s < g.start[l]) --l;
    q.l = l;
    const int p = s - g.start[l], W = g.W[l];
    const int y = p / W, x = p - y * W;
    q.ey = (float)cy[tok];
    q.ex = (float)cx[tok];
    if (normalize) {
        const float toty = (float)ty[(long long)q.n * g.SW + g.xoff[l] + x], totx = (float)tx[(long long)q.n * g.SH + g.yoff[l] + y];
        q.ey = q.ey / (toty + 1e-6f) * scale;
        q.ex = q.ex / (totx + 1e-6f) * scale;
    }
    return q;
}

// sin and cos of the pair of channels (c, c + 1), c even: channel c < F is the y half
__device__ __forceinline__ void sine_pair(const Geo &g, const Coord &q, const int c, const float *__restrict__ dim_t, float *s,
                                          float *co)
{
    const int F = g.C >> 1;
    const bool y_half = c < F;
    const float a = (y_half ? q.ey : q.ex) / dim_t[y_half ? c : c - F];
    sincosf(a, s, co);
}

__device__ __forceinline__ float round_to(const float v, const int code)
{
    if (code == kBF16) return __bfloat162float(__float2bfloat16(v));
    if (code == kF16) return __half2float(__float2half(v));
    return v;
}

__device__ __forceinline__ float embedded(float v, const Coord &q, const int c, const int C, const float *__restrict__ level_embed,
                                          const float *__restrict__ temporal_embed, const int round_dtype)
{
    if (temporal_embed) v = v + temporal_embed[(long long)q.n * C + c];
    v = round_to(v, round_dtype);
    return v + level_embed[q.l * C + c];
}

// The output as one dense array of `total` = N * S * C elements: a lane owns VEC of them, 16 bytes.
template <typename T>
__global__ __launch_bounds__(kThreads) void write_flat_kernel(const Geo g, const int *__restrict__ cy, const int *__restrict__ cx,
                                                              const int *__restrict__ ty, const int *__restrict__ tx,
                                                              const float *__restrict__ dim_t, const float *__restrict__ level_embed,
                                                              const float *__restrict__ temporal_embed, const int normalize,
                                                              const float scale, const int round_dtype, T *__restrict__ pos,
                                                              const long long total)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    const long long e0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * VEC;
    if (e0 >= total) return;
    const int count = total - e0 < VEC ? (int)(total - e0) : VEC;         // (even: C is)
    int tok = (int)(e0 / g.C), c = (int)(e0 - (long long)tok * g.C), have = -1;
    Coord q;
    alignas(16) T vals[VEC];
#pragma unroll
    for (int i = 0; i < VEC; i += 2) {
        if (i < count) {
            if (tok != have) {
                q = coord_of(g, tok, cy, cx, ty, tx, normalize, scale);
                have = tok;
            }
            float s, co;
            sine_pair(g, q, c, dim_t, &s, &co);
            from_acc(vals[i], embedded(s, q, c, g.C, level_embed, temporal_embed, round_dtype));
            from_acc(vals[i + 1], embedded(co, q, c + 1, g.C, level_embed, temporal_embed, round_dtype));
            c += 2;
            if (c >= g.C) {
                c = 0;
                ++tok;
            }
        }
    }
    if (count == VEC) {
        *reinterpret_cast<uint4 *>(pos + e0) = *reinterpret_cast<const uint4 *>(vals);
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            if (i < count) pos[e0 + i] = vals[i];          // the scalar tail
    }
}

// [N, C, H, W] of one level: a lane per (n, pair of channels, y, x), lanes along x.
template <typename T>
__global__ __launch_bounds__(kThreads) void write_nchw_kernel(const Geo g, const int *__restrict__ cy, const int *__restrict__ cx,
                                                              const int *__restrict__ ty, const int *__restrict__ tx,
                                                              const float *__restrict__ dim_t, const int normalize,
                                                              const float scale, T *__restrict__ pos, const long long total)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int pairs = g.C >> 1;
    const long long plane = i / g.S;                // n * pairs + pair
    const int p = (int)(i - plane * g.S);
    const int n = (int)(plane / pairs), c = 2 * (int)(plane - (long long)n * pairs);
    const Coord q = coord_of(g, n * g.S + p, cy, cx, ty, tx, normalize, scale);
    float s, co;
    sine_pair(g, q, c, dim_t, &s, &co);
    const long long at = ((long long)n * g.C + c) * g.S + p;
    from_acc(pos[at], s);
    from_acc(pos[at + g.S], co);
}

// ---- backward ------------------------------------------------------------------------------------------------------------
// partial[n, q, c]: the sum of grad over the tokens of chunk q of frame n, channel c.  Wave w adds the tokens w, w + 4, ...
// ascending; the waves are added ascending.
template <typename T>
__global__ __launch_bounds__(kThreads) void partial_kernel(const T *__restrict__ grad, const Geo g, const Chunks ch,
                                                           const int channel_blocks, float *__restrict__ partial)
{
    __shared__ float red[kWaves][kChunkChannels];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cb = blockIdx.x % channel_blocks;
    const int rest = blockIdx.x / channel_blocks;
    const int q = rest % ch.per_frame, n = rest / ch.per_frame;
    int l = g.L - 1;
    while (l > 0 && q < ch.first[l]) --l;
    const int t0 = (q - ch.first[l]) * kChunkTokens;
    const int left = g.H[l] * g.W[l] - t0;
    const int tokens = left < kChunkTokens ? left : kChunkTokens;
    const int c = cb * kChunkChannels + lane;
    float acc = 0.0f;
    if (c < g.C) {
        const T *src = grad + ((long long)n * g.S + g.start[l] + t0) * g.C + c;
        for (int t = wave; t < tokens; t += kWaves) acc += to_acc(src[(long long)t * g.C]);
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && c < g.C) {
        float v = red[0][lane];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v += red[w][lane];
        partial[((long long)n * ch.per_frame + q) * g.C + c] = v;
    }
}

// S[n, l, c]: the chunks of (n, l) ascending
__device__ __forceinline__ float segment_sum(const float *__restrict__ partial, const Geo &g, const Chunks &ch, const int n,
                                             const int l, const int c)
{
    const float *src = partial + ((long long)n * ch.per_frame + ch.first[l]) * g.C + c;
    float s = 0.0f;
    for (int j = 0; j < ch.count[l]; ++j) s += src[(long long)j * g.C];
    return s;
}

// Rows [0, L) of the grid are grad_level_embed, rows [L, L + N) grad_temporal_embed; a lane per channel.
__global__ __launch_bounds__(kThreads) void combine_kernel(const float *__restrict__ partial, const Geo g, const Chunks ch,
                                                           const int channel_blocks, float *__restrict__ grad_level_embed,
                                                           float *__restrict__ grad_temporal_embed)
{
    const int c = (blockIdx.x % channel_blocks) * kThreads + threadIdx.x;
    const int row = blockIdx.x / channel_blocks;
    if (c >= g.C) return;
    float acc = 0.0f;
    if (row < g.L) {
        if (!grad_level_embed) return;
        for (int n = 0; n < g.N; ++n) acc += segment_sum(partial, g, ch, n, row, c);
        grad_level_embed[row * g.C + c] = acc;
    } else {
        if (!grad_temporal_embed) return;
        const int n = row - g.L;
        for (int i = 0; i < g.L; ++i) acc += segment_sum(partial, g, ch, n, ch.order[i], c);
        grad_temporal_embed[(long long)n * g.C + c] = acc;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
inline long long align256(long long v) { return (v + 255) / 256 * 256; }

int check_shape(const posembed_shape *s, bool need_channels)
{
    if (!s) return err.fail("null pointer: shape");
    if (s->N < 0) return err.fail("N must not be negative");
    if (s->L < 1 || s->L > kMaxLevels) return err.fail("L = %lld is outside [1, %lld]", s->L, kMaxLevels);
    long long tokens = 0;
    for (int l = 0; l < s->L; ++l) {
        if (s->H[l] < 1 || s->W[l] < 1) return err.fail("H and W of level %lld must be positive", l);
        tokens += (long long)s->H[l] * s->W[l];
        if (tokens > 0x7fffffffLL) return err.fail("the tokens of a frame do not fit 31 bits");
    }
    if (tokens * (s->N > 0 ? s->N : 1) > 0x7fffffffLL) return err.fail("N * S = %lld does not fit 31 bits", tokens * s->N);
    if (need_channels && (s->C < 2 || s->C % 4 != 0))
        return err.fail("C = %lld must be 2 * num_pos_feats with an even, positive num_pos_feats", s->C);
    return POSEMBED_OK;
}

Geo geometry_of(const posembed_shape &s)
{
    Geo g = {};
    g.N = s.N, g.L = s.L, g.C = s.C;
    for (int l = 0; l < s.L; ++l) {
        g.H[l] = s.H[l], g.W[l] = s.W[l];
        g.start[l] = g.S, g.xoff[l] = g.SW, g.yoff[l] = g.SH;
        g.S += s.H[l] * s.W[l], g.SW += s.W[l], g.SH += s.H[l];
    }
    const long long per_pixel = align256((long long)s.N * g.S * 4);
    g.off_cx = per_pixel;
    g.off_ty = 2 * per_pixel;
    g.off_tx = g.off_ty + align256((long long)s.N * g.SW * 4);
    g.counts_bytes = g.off_tx + align256((long long)s.N * g.SH * 4);
    return g;
}

Chunks chunks_of(const posembed_shape &s)
{
    Chunks ch = {};
    for (int l = 0; l < s.L; ++l) {
        ch.first[l] = ch.per_frame;
        ch.count[l] = (int)cdiv((long long)s.H[l] * s.W[l], kChunkTokens);
        ch.per_frame += ch.count[l];
        // insertion by descending H * W, then H; equal levels keep the order of the call
        int at = l;
        while (at > 0) {
            const int o = ch.order[at - 1];
            const long long mine = (long long)s.H[l] * s.W[l], theirs = (long long)s.H[o] * s.W[o];
            if (theirs > mine || (theirs == mine && s.H[o] >= s.H[l])) break;
            ch.order[at] = o;
            --at;
        }
        ch.order[at] = l;
    }
    return ch;
}

struct CountPointers {
    int *cy, *cx, *ty, *tx;
};

CountPointers pointers_of(const Geo &g, const void *workspace)
{
    unsigned char *ws = (unsigned char *)workspace;
    return {(int *)ws, (int *)(ws + g.off_cx), (int *)(ws + g.off_ty), (int *)(ws + g.off_tx)};
}

int check_write(int dtype, const posembed_shape *shape, int normalize, float scale)
{
    if (dtype != kF32 && dtype != kBF16 && dtype != kF16) return err.fail("bad dtype code %lld (float32, bfloat16 or float16)", dtype);
    if (check_shape(shape, true) != POSEMBED_OK) return POSEMBED_ERR_ARGUMENT;
    if (normalize && !(scale == scale)) return err.fail("scale must be a number");
    return POSEMBED_OK;
}

// f(Tag<T>) for the three output types
template <typename F> int dispatch_out(int dtype, F &&f)
{
    switch (dtype) {
    case kF32: return f(Tag<float>());
    case kBF16: return f(Tag<__hip_bfloat16>());
    default: return f(Tag<__half>());
    }
}

}  // namespace posembed

using namespace posembed;

extern "C" {

int posembed_version(void) { return POSEMBED_ABI_VERSION; }

const char *posembed_last_error(void) { return err.msg; }

int posembed_tile(int which)
{
    switch (which) {
    case POSEMBED_TILE_TOKENS: return kChunkTokens;
    case POSEMBED_TILE_CHANNELS: return kChunkChannels;
    case POSEMBED_TILE_PIXELS: return 64;
    default: return -1;
    }
}

long long posembed_workspace_bytes(int which, const posembed_shape *shape)
{
    err.clear();
    if (which != POSEMBED_WS_COUNTS && which != POSEMBED_WS_BACKWARD) return err.fail("bad workspace code %lld", which);
    if (check_shape(shape, which == POSEMBED_WS_BACKWARD) != POSEMBED_OK) return POSEMBED_ERR_ARGUMENT;
    if (which == POSEMBED_WS_COUNTS) return geometry_of(*shape).counts_bytes;
    return align256((long long)shape->N * chunks_of(*shape).per_frame * shape->C * 4);
}

int posembed_counts(const posembed_masks *masks, const posembed_shape *shape, void *workspace, unsigned char *mask_flatten,
                    float *valid_ratios, void *stream)
{
    err.clear();
    if (check_shape(shape, false) != POSEMBED_OK) return POSEMBED_ERR_ARGUMENT;
    if (!masks) return err.fail("null pointer: masks");
    if (shape->N == 0) return POSEMBED_OK;
    for (int l = 0; l < shape->L; ++l)
        if (!masks->ptr[l]) return err.fail("null pointer: the mask of level %lld", l);
    if (!workspace) return err.fail("null pointer: workspace");
    const Geo g = geometry_of(*shape);
    CountJobs jobs = {};
    for (int l = 0; l < g.L; ++l) {
        jobs.rows[l] = (int)cdiv(g.H[l], kWaves);
        jobs.cols[l] = (int)cdiv(g.W[l], kThreads);
        jobs.per_frame += jobs.rows[l] + jobs.cols[l];
    }
    unsigned grid;
    if (err.grid_of((long long)g.N * jobs.per_frame, &grid) != kOk) return POSEMBED_ERR_ARGUMENT;
    const CountPointers p = pointers_of(g, workspace);
    hipLaunchKernelGGL(counts_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, *masks, g, jobs, p.cy, p.cx, p.ty, p.tx,
                       mask_flatten, valid_ratios);
    return err.check_launch("posembed_counts");
}

int posembed_write_flat(int dtype, const void *workspace, const posembed_shape *shape, const float *dim_t,
                        const float *level_embed, const float *temporal_embed, int normalize, float scale, int round_dtype,
                        void *pos, void *stream)
{
    err.clear();
    if (check_write(dtype, shape, normalize, scale) != POSEMBED_OK) return POSEMBED_ERR_ARGUMENT;
    if (round_dtype != POSEMBED_NO_ROUNDING && round_dtype != kBF16 && round_dtype != kF16)
        return err.fail("bad round_dtype code %lld (bfloat16, float16 or none)", round_dtype);
    if (shape->N == 0) return POSEMBED_OK;
    if (!workspace || !dim_t || !level_embed || !pos)
        return err.fail("null pointer: workspace, dim_t, level_embed and pos are required");
    if ((uintptr_t)pos % 16) return err.fail("pos must be 16-byte aligned");
    const Geo g = geometry_of(*shape);
    const CountPointers p = pointers_of(g, workspace);
    const long long total = (long long)g.N * g.S * g.C;
    return dispatch_out(dtype, [&](auto t) {
        typedef type_of<decltype(t)> T;
        unsigned grid;
        if (err.grid_of(cdiv(cdiv(total, 16 / (int)sizeof(T)), kThreads), &grid) != kOk) return (int)POSEMBED_ERR_ARGUMENT;
        hipLaunchKernelGGL((write_flat_kernel<T>), dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, g, p.cy, p.cx, p.ty, p.tx,
                           dim_t, level_embed, temporal_embed, normalize, scale, round_dtype, (T *)pos, total);
        return err.check_launch("posembed_write_flat");
    });
}

int posembed_write_nchw(int dtype, const void *workspace, const posembed_shape *shape, const float *dim_t, int normalize,
                        float scale, void *pos, void *stream)
{
    err.clear();
    if (check_write(dtype, shape, normalize, scale) != POSEMBED_OK) return POSEMBED_ERR_ARGUMENT;
    if (shape->L != 1) return err.fail("the nchw layout is one level, not %lld", shape->L);
    if (shape->N == 0) return POSEMBED_OK;
    if (!workspace || !dim_t || !pos) return err.fail("null pointer: workspace, dim_t and pos are required");
    const Geo g = geometry_of(*shape);
    const CountPointers p = pointers_of(g, workspace);
    const long long total = (long long)g.N * (g.C / 2) * g.S;
    return dispatch_out(dtype, [&](auto t) {
        typedef type_of<decltype(t)> T;
        unsigned grid;
        if (err.grid_of(cdiv(total, kThreads), &grid) != kOk) return (int)POSEMBED_ERR_ARGUMENT;
        hipLaunchKernelGGL((write_nchw_kernel<T>), dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, g, p.cy, p.cx, p.ty, p.tx,
                           dim_t, normalize, scale, (T *)pos, total);
        return err.check_launch("posembed_write_nchw");
    });
}

int posembed_backward(int dtype, const void *grad, const posembed_shape *shape, void *workspace, float *grad_level_embed,
                      float *grad_temporal_embed, void *stream)
{
    err.clear();
    if (check_write(dtype, shape, 0, 0.0f) != POSEMBED_OK) return POSEMBED_ERR_ARGUMENT;
    if (!grad_level_embed && !grad_temporal_embed) return err.fail("null pointer: one of the two gradients is required");
    const Geo g = geometry_of(*shape);
    const Chunks ch = chunks_of(*shape);
    if (g.N > 0 && (!grad || !workspace)) return err.fail("null pointer: grad and workspace are required");
    hipStream_t st = (hipStream_t)stream;
    if (g.N > 0) {
        const int blocks = (int)cdiv(g.C, kChunkChannels);
        unsigned grid;
        if (err.grid_of((long long)g.N * ch.per_frame * blocks, &grid) != kOk) return POSEMBED_ERR_ARGUMENT;
        const int rc = dispatch_out(dtype, [&](auto t) {
            typedef type_of<decltype(t)> T;
            hipLaunchKernelGGL((partial_kernel<T>), dim3(grid), dim3(kThreads), 0, st, (const T *)grad, g, ch, blocks,
                               (float *)workspace);
            return err.check_launch("posembed_backward");
        });
        if (rc != POSEMBED_OK) return rc;
    }
    const int blocks = (int)cdiv(g.C, kThreads);
    unsigned rows;
    if (err.grid_of(((long long)g.L + g.N) * blocks, &rows) != kOk) return POSEMBED_ERR_ARGUMENT;
    hipLaunchKernelGGL(combine_kernel, dim3(rows), dim3(kThreads), 0, st, (const float *)workspace, g, ch, blocks,
                       grad_level_embed, grad_temporal_embed);
    return err.check_launch("posembed_backward");
}

}  // extern "C"
