// frozennorm.hip -- the glue of the ResNet backbone's blocks (include/frozennorm.h): the frozen norm's
// affine map with the ReLU, the shortcut add (the downsample branch's norm folded in) and the stem's max-pool, forward and
// backward, each one pass.  gfx950, wave64, plain HIP.  Memory-bound streaming: 16-byte accesses where pointers and extents
// allow, the per-channel constants built in the kernel; there is no LDS, no atomic and no reduction.
#include "op_common.h"       // (fp contraction off)
#include "frozennorm.h"

namespace frozennorm {

using namespace devis;

static_assert(FROZENNORM_OK == kOk && FROZENNORM_ERR_ARGUMENT == kErrArgument && FROZENNORM_ERR_HIP == kErrHip, "status codes");
static_assert(FROZENNORM_F32 == kF32 && FROZENNORM_BF16 == kBF16 && FROZENNORM_F16 == kF16, "dtype codes");

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kUnroll = 4;              // NCHW: vectors a lane has in flight per stream
constexpr int kRowUnroll = 2;           // NHWC: rows a lane has in flight per stream
constexpr int kRowBlocks = 2048;        // NHWC: the most workgroups of a launch (eight per CU), which loop over the rows

thread_local Status err;     // frozennorm_last_error()

// what the kernels know of a call (host: geo_of)
struct Geo {
    long long N, planes, P, rows;       // planes = N * C of P = H * W elements; rows = N * H * W of C
    int C, H, W, layout, form, relu;
};

struct Norm {
    const float *w, *b, *m, *v;
    float eps;
};

// ---- the rule --------------------------------------------------------------------------------------------------------------
struct Consts {
    float s1, t1, s2, t2;
};

__device__ __forceinline__ float scale_of(const Norm &n, int c) { return n.w[c] * (1.0f / sqrtf(n.v[c] + n.eps)); }

// the constants of channel c; a backward needs the scales alone (and is given no bias or mean)
template <bool BWD> __device__ __forceinline__ Consts consts_of(const Norm &n1, const Norm &n2, int c, int form)
{
    Consts k = {1.0f, 0.0f, 1.0f, 0.0f};
    if (n1.w) {
        k.s1 = scale_of(n1, c);
        if (!BWD) k.t1 = n1.b[c] - n1.m[c] * k.s1;
    }
    if (form == FROZENNORM_NORMED && n2.w) {
        k.s2 = scale_of(n2, c);
        if (!BWD) k.t2 = n2.b[c] - n2.m[c] * k.s2;
    }
    return k;
}

__device__ __forceinline__ float relu_of(float z) { return z > 0.0f ? z : (z == z ? 0.0f : z); }

// forward: a = x, b = r -> o1 = y.  backward: a = grad_y, b = y -> o1 = grad_x, o2 = grad_r.
template <bool BWD>
__device__ __forceinline__ void compute(float a, float b, const Consts &k, int form, int relu, float &o1, float &o2)
{
    if (!BWD) {
        float z = fmaf(a, k.s1, k.t1);
        if (form == FROZENNORM_PLAIN) z = z + b;
        else if (form == FROZENNORM_NORMED) z = z + fmaf(b, k.s2, k.t2);
        o1 = relu ? relu_of(z) : z;
        o2 = 0.0f;
    } else {
        const float g = (!relu || b > 0.0f) ? a : 0.0f;
        o1 = g * k.s1;
        o2 = form == FROZENNORM_NORMED ? g * k.s2 : g;
    }
}

// ---- V consecutive elements ------------------------------------------------------------------------------------------------
template <typename T, int V> struct alignas(sizeof(T) * V >= 16 ? 16 : sizeof(T) * V) Pack {
    T v[V];
};

template <typename T, int V> __device__ __forceinline__ Pack<T, V> load_pack(const T *p)
{
    return *reinterpret_cast<const Pack<T, V> *>(p);
}

template <typename T, int V> __device__ __forceinline__ void store_pack(T *p, const float (&in)[V])
{
    Pack<T, V> q;
#pragma unroll
    for (int e = 0; e < V; ++e) from_acc(q.v[e], in[e]);
    *reinterpret_cast<Pack<T, V> *>(p) = q;
}

// ---- NCHW: a wave owns a unit of one plane -----------------------------------------------------------------------------------
// A plane of P elements starting at element `start` is a head up to the next multiple of V (the 16-byte grid: every pointer is
// 16-byte aligned when V > 1), a body of vectors and a tail; unit u of the plane takes the body's vectors [u, u + 1) * 64 *
// kUnroll, and unit 0 also the head and the tail, one element per lane.  V == 1 is the per-element path.  b, o1 and o2 may be
// NULL.
template <typename TA, typename TB, typename TO1, typename TO2, int V, bool BWD>
__global__ __launch_bounds__(kThreads) void nchw_kernel(const TA *__restrict__ a, const TB *__restrict__ b, TO1 *__restrict__ o1,
                                                        TO2 *__restrict__ o2, Norm n1, Norm n2, long long planes, int C,
                                                        long long P, int units, int form, int relu)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const long long unit = (long long)blockIdx.x * kWaves + wave;
    if (unit >= planes * units) return;
    const long long plane = unit / units;
    const int u = (int)(unit - plane * units);
    const Consts k = consts_of<BWD>(n1, n2, (int)(plane % C), form);
    const long long start = plane * P;
    long long head = V == 1 ? 0 : (long long)((V - (int)(start & (V - 1))) & (V - 1));
    if (head > P) head = P;
    const long long nvec = (P - head) / V, tail = head + nvec * V;
    const long long body = start + head;
    const long long i0 = (long long)u * (64 * kUnroll) + lane;
    Pack<TA, V> pa[kUnroll];
    Pack<TB, V> pb[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
        const long long i = i0 + j * 64;
        if (i < nvec) {
            pa[j] = load_pack<TA, V>(a + body + i * V);
            if (b) pb[j] = load_pack<TB, V>(b + body + i * V);
        }
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
        const long long i = i0 + j * 64;
        if (i < nvec) {
            float r1[V], r2[V];
#pragma unroll
            for (int e = 0; e < V; ++e) compute<BWD>(to_acc(pa[j].v[e]), b ? to_acc(pb[j].v[e]) : 0.0f, k, form, relu, r1[e], r2[e]);
            if (o1) store_pack<TO1, V>(o1 + body + i * V, r1);
            if (o2) store_pack<TO2, V>(o2 + body + i * V, r2);
        }
    }
    if (V > 1 && u == 0) {
        const long long edge = head + (P - tail);       // fewer than 2 V <= 16 elements
        if (lane < edge) {
            const long long at = start + (lane < head ? (long long)lane : tail + (lane - head));
            float r1, r2;
            compute<BWD>(to_acc(a[at]), b ? to_acc(b[at]) : 0.0f, k, form, relu, r1, r2);
            if (o1) from_acc(o1[at], r1);
            if (o2) from_acc(o2[at], r2);
        }
    }
}

// ---- NHWC: a lane owns V channels and walks the rows -------------------------------------------------------------------------
// A workgroup is (256 >> tw) rows of (1 << tw) lanes; lane column q of grid.y tile ty owns the channels (ty << tw | q) * V ..
// + V and keeps their constants in registers while the workgroup strides over the rows.  V > 1 needs C % V == 0 and 16-byte
// aligned pointers.
template <typename TA, typename TB, typename TO1, typename TO2, int V, bool BWD>
__global__ __launch_bounds__(kThreads) void nhwc_kernel(const TA *__restrict__ a, const TB *__restrict__ b, TO1 *__restrict__ o1,
                                                        TO2 *__restrict__ o2, Norm n1, Norm n2, long long rows, int C, int tw,
                                                        int form, int relu)
{
    const int t = threadIdx.x;
    const long long ch = ((long long)blockIdx.y << tw | (t & ((1 << tw) - 1))) * V;
    if (ch >= C) return;
    Consts k[V];
#pragma unroll
    for (int e = 0; e < V; ++e) k[e] = consts_of<BWD>(n1, n2, (int)ch + e, form);
    const int per = kThreads >> tw;
    const long long stride = (long long)gridDim.x * per;
    for (long long row = (long long)blockIdx.x * per + (t >> tw); row < rows; row += stride * kRowUnroll) {
        Pack<TA, V> pa[kRowUnroll];
        Pack<TB, V> pb[kRowUnroll];
#pragma unroll
        for (int j = 0; j < kRowUnroll; ++j) {
            const long long rr = row + j * stride;
            if (rr < rows) {
                pa[j] = load_pack<TA, V>(a + rr * C + ch);
                if (b) pb[j] = load_pack<TB, V>(b + rr * C + ch);
            }
        }
#pragma unroll
        for (int j = 0; j < kRowUnroll; ++j) {
            const long long rr = row + j * stride;
            if (rr < rows) {
                float r1[V], r2[V];
#pragma unroll
                for (int e = 0; e < V; ++e)
                    compute<BWD>(to_acc(pa[j].v[e]), b ? to_acc(pb[j].v[e]) : 0.0f, k[e], form, relu, r1[e], r2[e]);
                if (o1) store_pack<TO1, V>(o1 + rr * C + ch, r1);
                if (o2) store_pack<TO2, V>(o2 + rr * C + ch, r2);
            }
        }
    }
}

// ---- the stem: affine, ReLU and the 3 x 3 / stride 2 / padding 1 maximum -----------------------------------------------------
__device__ __forceinline__ void pool_tap(float &best, float x, float s, float t)
{
    const float v = relu_of(fmaf(x, s, t));
    if (v > best || v != v) best = v;
}

// a workgroup owns 256 consecutive outputs of one plane (its constants are uniform); one output per lane, read per element
template <typename TX, typename TY>
__global__ __launch_bounds__(kThreads) void pool_nchw_kernel(const TX *__restrict__ x, TY *__restrict__ y, Norm n, int C, int H,
                                                             int W, int Ho, int Wo, int chunks)
{
    const long long plane = blockIdx.x / chunks;
    const long long idx = (long long)(blockIdx.x - plane * chunks) * kThreads + threadIdx.x;
    const long long Po = (long long)Ho * Wo;
    if (idx >= Po) return;
    const int c = (int)(plane % C);
    const float s = scale_of(n, c), t = n.b[c] - n.m[c] * s;
    const int ho = (int)(idx / Wo), wo = (int)(idx - (long long)ho * Wo);
    const TX *src = x + plane * ((long long)H * W);
    float best = -INFINITY;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const long long h = 2LL * ho + dy;
        if (h < 0 || h >= H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const long long w = 2LL * wo + dx;
            if (w < 0 || w >= W) continue;
            pool_tap(best, to_acc(src[h * W + w]), s, t);
        }
    }
    from_acc(y[plane * Po + idx], best);
}

// nhwc_kernel's ownership over the OUTPUT rows (n, ho, wo); a tap is one pack of V channels
template <typename TX, typename TY, int V>
__global__ __launch_bounds__(kThreads) void pool_nhwc_kernel(const TX *__restrict__ x, TY *__restrict__ y, Norm n, long long rows,
                                                             int C, int H, int W, int Ho, int Wo, int tw)
{
    const int t = threadIdx.x;
    const long long ch = ((long long)blockIdx.y << tw | (t & ((1 << tw) - 1))) * V;
    if (ch >= C) return;
    float s[V], b[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        s[e] = scale_of(n, (int)ch + e);
        b[e] = n.b[ch + e] - n.m[ch + e] * s[e];
    }
    const int per = kThreads >> tw;
    const long long stride = (long long)gridDim.x * per;
    for (long long row = (long long)blockIdx.x * per + (t >> tw); row < rows; row += stride) {
        const long long q = row / Wo;
        const int wo = (int)(row - q * Wo);
        const long long nb = q / Ho;
        const int ho = (int)(q - nb * Ho);
        float best[V];
#pragma unroll
        for (int e = 0; e < V; ++e) best[e] = -INFINITY;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const long long h = 2LL * ho + dy;
            if (h < 0 || h >= H) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const long long w = 2LL * wo + dx;
                if (w < 0 || w >= W) continue;
                const Pack<TX, V> p = load_pack<TX, V>(x + ((nb * H + h) * W + w) * C + ch);
#pragma unroll
                for (int e = 0; e < V; ++e) pool_tap(best[e], to_acc(p.v[e]), s[e], b[e]);
            }
        }
        store_pack<TY, V>(y + row * C + ch, best);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
bool is16(int d) { return d == kBF16 || d == kF16; }
bool known(int d) { return d == kF32 || is16(d); }

int check_types(const frozennorm_types *t, int form)
{
    if (!t) return err.fail("null pointer: types");
    if (!known(t->x) || !known(t->r) || !known(t->y))
        return err.fail("bad dtype code (float32, bfloat16 and float16 are the kernels' dtypes)");
    const int codes[3] = {t->x, t->r, t->y};
    int half = 0;
    for (int code : codes) {
        if (!is16(code)) continue;
        if (half && half != code) return err.fail("bad dtype mix: bfloat16 and float16 do not meet in one call");
        half = code;
    }
    if (form == FROZENNORM_NONE && t->r != t->x) return err.fail("without a residual, types.r must equal types.x");
    return FROZENNORM_OK;
}

int geo_of(const frozennorm_shape *s, Geo *geo)
{
    if (!s) return err.fail("null pointer: shape");
    if (s->layout != FROZENNORM_NCHW && s->layout != FROZENNORM_NHWC) return err.fail("bad layout %lld", s->layout);
    if (s->residual != FROZENNORM_NONE && s->residual != FROZENNORM_PLAIN && s->residual != FROZENNORM_NORMED)
        return err.fail("bad residual form %lld", s->residual);
    if (s->relu != 0 && s->relu != 1) return err.fail("relu must be 0 or 1, got %lld", s->relu);
    if (s->N < 0 || s->H < 0 || s->W < 0) return err.fail("N, H and W must not be negative");
    if (s->C < 1) return err.fail("C must be positive, got %lld", s->C);
    if (s->N > 0x7fffffffLL) return err.fail("N = %lld does not fit 31 bits", s->N);
    geo->N = s->N, geo->C = s->C, geo->H = s->H, geo->W = s->W;
    geo->layout = s->layout, geo->form = s->residual, geo->relu = s->relu;
    geo->P = (long long)s->H * s->W;
    geo->planes = s->N * s->C;
    if (geo->P > 0 && geo->planes > (1LL << 62) / geo->P) return err.fail("too many elements for 64-bit offsets");
    geo->rows = s->N * geo->P;
    return FROZENNORM_OK;
}

// the device view of a norm; `full` asks for bias and mean too
int norm_of(const frozennorm_norm *n, bool full, const char *which, Norm *out)
{
    if (!n) return err.fail(which[0] == 'r' ? "null pointer: norm_r is required" : "null pointer: norm is required");
    if (!n->weight || !n->var || (full && (!n->bias || !n->mean)))
        return err.fail(which[0] == 'r' ? "null pointer: a buffer of norm_r" : "null pointer: a buffer of norm");
    if (!(n->eps == n->eps)) return err.fail("eps must be a number");
    out->w = n->weight, out->b = n->bias, out->m = n->mean, out->v = n->var, out->eps = (float)n->eps;
    return FROZENNORM_OK;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }       // (NULL is aligned)

// f(Tag<TX>, Tag<TR>, Tag<TY>) of a checked combination
template <typename H, typename F> int pick(int code, F &&f) { return code == kF32 ? f(Tag<float>()) : f(Tag<H>()); }

template <typename H, typename F> int dispatch16(const frozennorm_types &t, F &&f)
{
    return pick<H>(t.x, [&](auto tx) {
        return pick<H>(t.r, [&](auto tr) { return pick<H>(t.y, [&](auto ty) { return f(tx, tr, ty); }); });
    });
}

template <typename F> int dispatch_types(const frozennorm_types &t, F &&f)
{
    const bool bf = t.x == kBF16 || t.r == kBF16 || t.y == kBF16;
    return bf ? dispatch16<__hip_bfloat16>(t, f) : dispatch16<__half>(t, f);
}

template <typename A, typename B, typename C> constexpr int width_of()
{
    return sizeof(A) == 4 && sizeof(B) == 4 && sizeof(C) == 4 ? 4 : 8;
}

// the lane columns of an NHWC launch: tw = log2 of the columns per workgroup, tiles = grid.y
int columns_of(int C, int V, int *tw, unsigned *tiles)
{
    const long long cols = C / V;
    int log = 0;
    while ((1 << log) < cols && (1 << log) < kThreads) ++log;
    const long long need = cdiv(cols, 1LL << log);
    if (need > 65535) return err.fail("C = %lld is more channels than one launch covers", C);
    *tw = log, *tiles = (unsigned)need;
    return FROZENNORM_OK;
}

// one elementwise launch.  forward: (a, b, o1, o2) = (x, r, y, NULL); backward: (grad_y, y, grad_x, grad_r)
template <bool BWD, typename TA, typename TB, typename TO1, typename TO2, int VW>
int launch(const Geo &geo, const void *a, const void *b, void *o1, void *o2, const Norm &n1, const Norm &n2, hipStream_t st,
           const char *what)
{
    const bool aligned = aligned16(a) && aligned16(b) && aligned16(o1) && aligned16(o2);
    if (geo.layout == FROZENNORM_NCHW) {
        const long long per = cdiv(geo.P, 64LL * kUnroll * (aligned ? VW : 1));       // (at least the body's vectors)
        if (per > 0x7fffffffLL) return err.fail("H * W = %lld is too large", geo.P);
        const int units = (int)(per > 0 ? per : 1);
        if (geo.planes > (1LL << 62) / units) return err.fail("too many workgroups for one launch");
        unsigned grid;
        if (err.grid_of(cdiv(geo.planes * units, kWaves), &grid) != FROZENNORM_OK) return FROZENNORM_ERR_ARGUMENT;
        if (aligned)
            hipLaunchKernelGGL((nchw_kernel<TA, TB, TO1, TO2, VW, BWD>), dim3(grid), dim3(kThreads), 0, st, (const TA *)a,
                               (const TB *)b, (TO1 *)o1, (TO2 *)o2, n1, n2, geo.planes, geo.C, geo.P, units, geo.form, geo.relu);
        else
            hipLaunchKernelGGL((nchw_kernel<TA, TB, TO1, TO2, 1, BWD>), dim3(grid), dim3(kThreads), 0, st, (const TA *)a,
                               (const TB *)b, (TO1 *)o1, (TO2 *)o2, n1, n2, geo.planes, geo.C, geo.P, units, geo.form, geo.relu);
        return err.check_launch(what);
    }
    const bool vec = aligned && geo.C % VW == 0;
    int tw;
    unsigned tiles;
    if (columns_of(geo.C, vec ? VW : 1, &tw, &tiles) != FROZENNORM_OK) return FROZENNORM_ERR_ARGUMENT;
    const long long want = cdiv(geo.rows, (long long)(kThreads >> tw) * kRowUnroll);
    const long long cap = kRowBlocks / tiles > 0 ? kRowBlocks / tiles : 1;
    const dim3 grid((unsigned)(want < cap ? want : cap), tiles);
    if (vec)
        hipLaunchKernelGGL((nhwc_kernel<TA, TB, TO1, TO2, VW, BWD>), grid, dim3(kThreads), 0, st, (const TA *)a, (const TB *)b,
                           (TO1 *)o1, (TO2 *)o2, n1, n2, geo.rows, geo.C, tw, geo.form, geo.relu);
    else
        hipLaunchKernelGGL((nhwc_kernel<TA, TB, TO1, TO2, 1, BWD>), grid, dim3(kThreads), 0, st, (const TA *)a, (const TB *)b,
                           (TO1 *)o1, (TO2 *)o2, n1, n2, geo.rows, geo.C, tw, geo.form, geo.relu);
    return err.check_launch(what);
}

}  // namespace frozennorm

using namespace frozennorm;

extern "C" {

int frozennorm_version(void) { return FROZENNORM_ABI_VERSION; }

const char *frozennorm_last_error(void) { return err.msg; }

int frozennorm_pooled_size(int n) { return n < 0 ? -1 : (n == 0 ? 0 : (n - 1) / 2 + 1); }

int frozennorm_forward(const frozennorm_types *types, const frozennorm_shape *shape, const void *x, const frozennorm_norm *norm,
                       const void *r, const frozennorm_norm *norm_r, void *y, void *stream)
{
    err.clear();
    Geo geo;
    if (geo_of(shape, &geo) != FROZENNORM_OK || check_types(types, geo.form) != FROZENNORM_OK) return FROZENNORM_ERR_ARGUMENT;
    Norm n1, n2 = {nullptr, nullptr, nullptr, nullptr, 0.0f};
    if (norm_of(norm, true, "norm", &n1) != FROZENNORM_OK) return FROZENNORM_ERR_ARGUMENT;
    if (geo.form == FROZENNORM_NORMED) {
        if (norm_of(norm_r, true, "r", &n2) != FROZENNORM_OK) return FROZENNORM_ERR_ARGUMENT;
    } else if (norm_r) {
        return err.fail("norm_r belongs to the normalised residual form");
    }
    if (geo.form == FROZENNORM_NONE && r) return err.fail("r is given without a residual form");
    if (!y) return err.fail("null pointer: y is required");
    if (geo.planes == 0 || geo.P == 0) return FROZENNORM_OK;
    if (!x) return err.fail("null pointer: x is required");
    if (geo.form != FROZENNORM_NONE && !r) return err.fail("null pointer: r is required in the residual forms");
    hipStream_t st = (hipStream_t)stream;
    return dispatch_types(*types, [&](auto tx, auto tr, auto ty) {
        typedef type_of<decltype(tx)> TX;
        typedef type_of<decltype(tr)> TR;
        typedef type_of<decltype(ty)> TY;
        return launch<false, TX, TR, TY, TY, width_of<TX, TR, TY>()>(geo, x, r, y, nullptr, n1, n2, st, "frozennorm_forward");
    });
}

int frozennorm_backward(const frozennorm_types *types, const frozennorm_shape *shape, const void *grad_y, const void *y,
                        const frozennorm_norm *norm, const frozennorm_norm *norm_r, void *grad_x, void *grad_r, void *stream)
{
    err.clear();
    Geo geo;
    if (geo_of(shape, &geo) != FROZENNORM_OK || check_types(types, geo.form) != FROZENNORM_OK) return FROZENNORM_ERR_ARGUMENT;
    if (!grad_x && !grad_r) return err.fail("no gradient is asked for");
    if (grad_r && geo.form == FROZENNORM_NONE) return err.fail("grad_r is asked for without a residual form");
    Norm n1 = {nullptr, nullptr, nullptr, nullptr, 0.0f}, n2 = n1;
    if (grad_x && norm_of(norm, false, "norm", &n1) != FROZENNORM_OK) return FROZENNORM_ERR_ARGUMENT;
    if (grad_r && geo.form == FROZENNORM_NORMED && norm_of(norm_r, false, "r", &n2) != FROZENNORM_OK) return FROZENNORM_ERR_ARGUMENT;
    if (geo.planes == 0 || geo.P == 0) return FROZENNORM_OK;
    if (!grad_y) return err.fail("null pointer: grad_y is required");
    if (geo.relu && !y) return err.fail("null pointer: y is required behind a ReLU");
    hipStream_t st = (hipStream_t)stream;
    return dispatch_types(*types, [&](auto tx, auto tr, auto ty) {
        typedef type_of<decltype(tx)> TX;
        typedef type_of<decltype(tr)> TR;
        typedef type_of<decltype(ty)> TY;
        return launch<true, TY, TY, TX, TR, width_of<TX, TR, TY>()>(geo, grad_y, geo.relu ? y : nullptr, grad_x, grad_r, n1, n2,
                                                                     st, "frozennorm_backward");
    });
}

int frozennorm_pool_forward(const frozennorm_types *types, const frozennorm_shape *shape, const void *x,
                            const frozennorm_norm *norm, void *y, void *stream)
{
    err.clear();
    Geo geo;
    if (geo_of(shape, &geo) != FROZENNORM_OK || check_types(types, geo.form) != FROZENNORM_OK) return FROZENNORM_ERR_ARGUMENT;
    if (geo.form != FROZENNORM_NONE) return err.fail("the pool has no residual form");
    if (types->r != types->x) return err.fail("without a residual, types.r must equal types.x");
    Norm n;
    if (norm_of(norm, true, "norm", &n) != FROZENNORM_OK) return FROZENNORM_ERR_ARGUMENT;
    if (!y) return err.fail("null pointer: y is required");
    if (geo.planes == 0 || geo.P == 0) return FROZENNORM_OK;
    if (!x) return err.fail("null pointer: x is required");
    const int Ho = frozennorm_pooled_size(geo.H), Wo = frozennorm_pooled_size(geo.W);
    const long long Po = (long long)Ho * Wo;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_types(*types, [&](auto tx, auto, auto ty) {
        typedef type_of<decltype(tx)> TX;
        typedef type_of<decltype(ty)> TY;
        constexpr int VW = width_of<TX, TX, TY>();
        if (geo.layout == FROZENNORM_NCHW) {
            const long long chunks = cdiv(Po, kThreads);
            unsigned grid;
            if (chunks > 0x7fffffffLL || err.grid_of(geo.planes * chunks, &grid) != FROZENNORM_OK)
                return err.fail("too many workgroups for one launch");
            hipLaunchKernelGGL((pool_nchw_kernel<TX, TY>), dim3(grid), dim3(kThreads), 0, st, (const TX *)x, (TY *)y, n, geo.C,
                               geo.H, geo.W, Ho, Wo, (int)chunks);
            return err.check_launch("frozennorm_pool_forward");
        }
        const bool vec = aligned16(x) && aligned16(y) && geo.C % VW == 0;
        const long long rows = geo.N * Po;
        int tw;
        unsigned tiles;
        if (columns_of(geo.C, vec ? VW : 1, &tw, &tiles) != FROZENNORM_OK) return (int)FROZENNORM_ERR_ARGUMENT;
        const long long want = cdiv(rows, kThreads >> tw);
        const long long cap = 4 * kRowBlocks / tiles > 0 ? 4 * kRowBlocks / tiles : 1;
        const dim3 grid((unsigned)(want < cap ? want : cap), tiles);
        if (vec)
            hipLaunchKernelGGL((pool_nhwc_kernel<TX, TY, VW>), grid, dim3(kThreads), 0, st, (const TX *)x, (TY *)y, n, rows, geo.C,
                               geo.H, geo.W, Ho, Wo, tw);
        else
            hipLaunchKernelGGL((pool_nhwc_kernel<TX, TY, 1>), grid, dim3(kThreads), 0, st, (const TX *)x, (TY *)y, n, rows, geo.C,
                               geo.H, geo.W, Ho, Wo, tw);
        return err.check_launch("frozennorm_pool_forward");
    });
}

}  // extern "C"
