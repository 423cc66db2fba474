// maskiou.hip -- the clip-stitching operators (include/maskiou.h): the matrix of soft mask IoUs between
// two sets of small logit maps as a split-K product whose operands -- sigmoid of the bilinearly resampled logits -- are built
// tile by tile in LDS and never exist in memory, and the binarised full-resolution masks, one byte per pixel.  gfx950, wave64,
// plain HIP; float arithmetic accumulates on the matrix pipe (the f32-input MFMA: exact f32, a k-ordered fma chain), double
// with explicit fma; no atomics: every sum has a fixed order.
//
// The kernels are templates of the storage type of the logits alone.
#include "op_common.h"       // (fp contraction off)
#include "mask_taps.h"
#include "maskiou.h"

namespace maskiou {

using namespace devis;

static_assert(MASKIOU_OK == kOk && MASKIOU_ERR_ARGUMENT == kErrArgument && MASKIOU_ERR_HIP == kErrHip, "status codes");
static_assert(MASKIOU_F32 == kF32 && MASKIOU_F64 == kF64 && MASKIOU_BF16 == kBF16 && MASKIOU_F16 == kF16, "dtype codes");

constexpr int kThreads = 256;
constexpr int kBlock = 64;                      // pairwise: rows of a and of b per workgroup
constexpr int kTH = 2, kTW = 16;                // pairwise: destination rows x columns of a pixel tile
constexpr int kKT = kTH * kTW;                  // pixels of a tile: the k extent of one LDS image
constexpr int kLd = 2 * kBlock + 1;             // row pitch of the LDS image [kKT][a's block | b's block], odd: no bank conflicts
constexpr int kSplitTiles = 4;                  // the fewest tiles of a split range
constexpr int kMaxSplits = 128;                 // the most split ranges of a frame
constexpr int kPer = 16;                        // binarise: consecutive bytes of out per lane (one 16-byte store)
constexpr int kBinTile = kThreads * kPer;
constexpr int kBinSrc = 4096;                  // binarise: source elements kept in LDS
static_assert(kKT == 32 && kThreads == 8 * kKT, "the p pass: 8 maps at a time, one pixel per lane of a half wave");
static_assert(kBlock == 64 && kThreads == 256, "four waves, one 32x32 quarter of the output block each");

typedef float floatx16 __attribute__((ext_vector_type(16)));

thread_local Status err;     // maskiou_last_error()

// (the resampling rule of include/maskloss.h -- Tap, tap_at, lerp_of, logit_at -- is mask_taps.h, shared with maskrle.hip)

template <typename A> __device__ __forceinline__ A sigmoid_of(A x)
{
    const A e = exp_of(-(x < (A)0 ? -x : x));
    const A inv = (A)1 / ((A)1 + e);
    return x >= (A)0 ? inv : e * inv;
}

// ---- how the k axis is cut: a function of (F, H, W) alone ---------------------------------------------------------------
struct Cut {
    int tiles_x, tiles;     // tile columns; tiles per frame
    int per, splits;        // tiles of a split range; split ranges per frame
};

inline Cut cut_of(const maskiou_shape &s)
{
    Cut c;
    c.tiles_x = (int)cdiv(s.W, kTW);
    c.tiles = (int)(cdiv(s.H, kTH) * c.tiles_x);
    const int even = (int)cdiv(c.tiles, kMaxSplits);
    c.per = even > kSplitTiles ? even : kSplitTiles;
    c.splits = (int)cdiv(c.tiles, c.per);
    return c;
}

__host__ __device__ inline long long entries_of(const maskiou_shape &s) { return (long long)s.Na * s.Nb + s.Na + s.Nb; }

// ---- pairwise ---------------------------------------------------------------------------------------------------------
// A workgroup owns a kBlock x kBlock block of (i, j), one frame and one split range of that frame's tiles.  Per tile: every
// thread evaluates p for one pixel of 16 of the block's 128 maps into the LDS image ps[pixel][map] (maps past Na / Nb and
// positions outside the frame are 0, which leaves every chain as it is); then the block's entries advance over the tile's 32
// pixels in ascending order -- float: wave v owns the 32x32 quarter (v >> 1, v & 1) and issues one 32x32x2 MFMA per pixel
// pair; double: a thread owns 4 x 4 entries and one fma per entry and pixel -- and the first 128 threads advance the sums of
// their map.  The range's partials go to ws[(f * S + split) * E + {i * Nb + j | Na*Nb + i | Na*Nb + Na + j}].
template <typename T>
__global__ __launch_bounds__(kThreads) void pairwise_kernel(const T *__restrict__ a, const T *__restrict__ b,
                                                            typename Acc<T>::type *__restrict__ ws, const maskiou_shape s,
                                                            const Cut c, const int BA, const int BB)
{
    typedef typename Acc<T>::type A;
    constexpr bool kMatrix = sizeof(A) == 4;
    __shared__ A ps[kKT * kLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long blk = blockIdx.x;
    const int bb = (int)(blk % BB);
    blk /= BB;
    const int ba = (int)(blk % BA);
    const long long fs = blk / BA;
    const int f = (int)(fs / c.splits), sp = (int)(fs % c.splits);
    const int t0 = sp * c.per, t1 = t0 + c.per < c.tiles ? t0 + c.per : c.tiles;
    const int p = s.h * s.w;
    const A scale_y = (A)s.h / (A)s.H, scale_x = (A)s.w / (A)s.W;
    const int px = tid & (kKT - 1), grp = tid >> 5;

    floatx16 macc;
    A acc[4][4];
#pragma unroll
    for (int r = 0; r < 16; ++r) macc[r] = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[r][q] = (A)0;
    A sacc = (A)0;

    for (int tile = t0; tile < t1; ++tile) {
        const int ty0 = tile / c.tiles_x, tx0 = tile - ty0 * c.tiles_x;
        const int y = ty0 * kTH + (px >> 4), x = tx0 * kTW + (px & 15);
        const bool inside = y < s.H && x < s.W;
        const Tap<A> ty = tap_at<A>(inside ? y : 0, s.h, scale_y), tx = tap_at<A>(inside ? x : 0, s.w, scale_x);
#pragma unroll 4
        for (int it = 0; it < 2 * kBlock / 8; ++it) {
            const int slot = grp + 8 * it;
            const bool of_a = slot < kBlock;
            const int m = of_a ? ba * kBlock + slot : bb * kBlock + slot - kBlock;
            A v = (A)0;
            if (inside && m < (of_a ? s.Na : s.Nb)) {
                const T *sp_ = (of_a ? a : b) + ((long long)m * s.F + f) * p;
                v = sigmoid_of(logit_at<T>(sp_, s.w, ty, tx));
            }
            ps[px * kLd + slot] = v;
        }
        __syncthreads();
        if constexpr (kMatrix) {
            const int ra = (wave >> 1) * 32 + (lane & 31), rb = kBlock + (wave & 1) * 32 + (lane & 31);
#pragma unroll
            for (int k = 0; k < kKT; k += 2) {
                const float *row = reinterpret_cast<const float *>(ps) + (k + (lane >> 5)) * kLd;
                macc = __builtin_amdgcn_mfma_f32_32x32x2f32(row[ra], row[rb], macc, 0, 0, 0);
            }
        } else {
            const int ti = tid >> 4, tj = tid & 15;
#pragma unroll 4
            for (int k = 0; k < kKT; ++k) {
                A av[4], bv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    av[r] = ps[k * kLd + ti + 16 * r];
                    bv[r] = ps[k * kLd + kBlock + tj + 16 * r];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[r][q] = fma_of(av[r], bv[q], acc[r][q]);
            }
        }
        if (tid < 2 * kBlock) {
#pragma unroll 8
            for (int k = 0; k < kKT; ++k) sacc += ps[k * kLd + tid];
        }
        __syncthreads();
    }

    A *dst = ws + fs * entries_of(s);
    if constexpr (kMatrix) {
        // C / D of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
        const int j = bb * kBlock + (wave & 1) * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = ba * kBlock + (wave >> 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (i < s.Na && j < s.Nb) dst[(long long)i * s.Nb + j] = macc[r];
        }
    } else {
        const int ti = tid >> 4, tj = tid & 15;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = ba * kBlock + ti + 16 * r, j = bb * kBlock + tj + 16 * q;
                if (i < s.Na && j < s.Nb) dst[(long long)i * s.Nb + j] = acc[r][q];
            }
    }
    A *sums = dst + (long long)s.Na * s.Nb;
    if (tid < kBlock) {
        const int i = ba * kBlock + tid;
        if (bb == 0 && i < s.Na) sums[i] = sacc;
    } else if (tid < 2 * kBlock) {
        const int j = bb * kBlock + tid - kBlock;
        if (ba == 0 && j < s.Nb) sums[s.Na + j] = sacc;
    }
}

// One thread per entry (i, j): per frame the split partials in ascending order -> inter, and from the threads of column 0 /
// row 0 sum_a / sum_b; then the ratio.
template <typename A>
__global__ __launch_bounds__(kThreads) void combine_kernel(const A *__restrict__ ws, A *__restrict__ inter, A *__restrict__ sum_a,
                                                           A *__restrict__ sum_b, A *__restrict__ iou, const maskiou_shape s,
                                                           const int splits, const int reduce, const A eps)
{
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long nn = (long long)s.Na * s.Nb, E = nn + s.Na + s.Nb;
    if (e >= nn) return;
    const int i = (int)(e / s.Nb), j = (int)(e - (long long)i * s.Nb);
    A I = (A)0, SA = (A)0, SB = (A)0, ratio = (A)0;
    for (int f = 0; f < s.F; ++f) {
        A If = (A)0, Af = (A)0, Bf = (A)0;
        const A *wp = ws + (long long)f * splits * E;
        for (int k = 0; k < splits; ++k, wp += E) {
            If += wp[e];
            Af += wp[nn + i];
            Bf += wp[nn + s.Na + j];
        }
        inter[f * nn + e] = If;
        if (j == 0) sum_a[(long long)f * s.Na + i] = Af;
        if (i == 0) sum_b[(long long)f * s.Nb + j] = Bf;
        I += If;
        SA += Af;
        SB += Bf;
        const A u = Af + Bf - If;
        ratio += If / (u < eps ? eps : u);
    }
    if (reduce == MASKIOU_FRAME) {
        iou[e] = ratio / (A)s.F;
    } else {
        const A u = SA + SB - I;
        iou[e] = I / (u < eps ? eps : u);
    }
}

// ---- binarise ---------------------------------------------------------------------------------------------------------
// A workgroup owns kBinTile consecutive bytes of one mask of `out`, a lane kPer of them: consecutive destination pixels of a
// row (row-major) or of a column (column-major).  Call the axis the bytes run along the inner one.  The tile is a few outer
// indices, so its taps touch a few source rows (row-major) or source columns (column-major): they are staged in LDS in the
// arithmetic type, as [outer source index][inner source index], when they fit kBinSrc elements (they do unless the map is
// downsampled steeply), else read from memory.  The inner axis's taps are formed per pixel, the outer axis's when the lane
// crosses into the next row / column.
template <typename T>
__global__ __launch_bounds__(kThreads) void binarize_kernel(const T *__restrict__ src, unsigned char *__restrict__ out,
                                                            const int h, const int w, const int H, const int W,
                                                            const int tiles, const int col_major)
{
    typedef typename Acc<T>::type A;
    __shared__ A rows[kBinSrc];
    const long long n = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles, tid = threadIdx.x;
    const int P = H * W;
    const int in_o = col_major ? w : h, out_o = col_major ? W : H, in_i = col_major ? h : w, out_i = col_major ? H : W;
    const A scale_o = (A)in_o / (A)out_o, scale_i = (A)in_i / (A)out_i;
    const T *sp = src + n * ((long long)h * w);
    const int base = tile * kBinTile;                   // (tile * kBinTile < P <= 2^31 - 1)
    const int end = P - base < kBinTile ? P : base + kBinTile;
    // the outer source indices of the tile's first and last destination row / column
    const int s0 = tap_at<A>(base / out_i, in_o, scale_o).i0, s1 = tap_at<A>((end - 1) / out_i, in_o, scale_o).i1;
    const bool staged = (long long)(s1 - s0 + 1) * in_i <= kBinSrc;
    if (staged) {
        const int cnt = (s1 - s0 + 1) * in_i;
        if (col_major) {
            const int cols = s1 - s0 + 1;               // consecutive threads read consecutive source columns
            for (int i = tid; i < cnt; i += kThreads) {
                const int y = i / cols, c = i - y * cols;
                rows[c * in_i + y] = (A)to_acc(sp[(long long)y * w + s0 + c]);
            }
        } else {
            for (int i = tid; i < cnt; i += kThreads) rows[i] = (A)to_acc(sp[(long long)s0 * w + i]);
        }
        __syncthreads();
    }
    const int q0 = base + tid * kPer;
    if (q0 >= end) return;
    int o = q0 / out_i, ii = q0 - o * out_i;
    Tap<A> to = tap_at<A>(o, in_o, scale_o);
    const int cnt = end - q0 < kPer ? end - q0 : kPer;
    unsigned int word[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        if (j < cnt) {
            const Tap<A> ti = tap_at<A>(ii, in_i, scale_i);
            A x;
            if (staged) {
                const A *ra = rows + (to.i0 - s0) * in_i, *rb = rows + (to.i1 - s0) * in_i;
                const A v00 = ra[ti.i0], vi = ra[ti.i1], vo = rb[ti.i0], v11 = rb[ti.i1];
                x = col_major ? lerp_of<A>(ti, to, v00, vo, vi, v11) : lerp_of<A>(to, ti, v00, vi, vo, v11);
            } else {
                x = col_major ? logit_at<T>(sp, w, ti, to) : logit_at<T>(sp, w, to, ti);
            }
            word[j >> 2] |= (x > (A)0 ? 1u : 0u) << ((j & 3) * 8);
            if (++ii == out_i) {
                ii = 0;
                ++o;
                if (o < out_o) to = tap_at<A>(o, in_o, scale_o);
            }
        }
    }
    unsigned char *op = out + n * P + q0;
    if (cnt == kPer && (reinterpret_cast<unsigned long long>(op) & 15ull) == 0) {
        *reinterpret_cast<uint4 *>(op) = make_uint4(word[0], word[1], word[2], word[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kPer; ++j)
            if (j < cnt) op[j] = (unsigned char)((word[j >> 2] >> ((j & 3) * 8)) & 0xffu);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------
int check_map(int h, int w, int H, int W)
{
    if (h <= 0 || w <= 0 || H <= 0 || W <= 0) return err.fail("sizes must be positive (the numbers of maps may be 0)");
    if ((long long)h * w > 0x7fffffffLL) return err.fail("h * w = %lld does not fit 31 bits", (long long)h * w);
    if ((long long)H * W > 0x7fffffffLL) return err.fail("H * W = %lld does not fit 31 bits", (long long)H * W);
    return MASKIOU_OK;
}

int check_shape(const maskiou_shape *s)
{
    if (!s) return err.fail("null pointer: shape");
    if (s->Na < 0 || s->Nb < 0 || s->F <= 0) return err.fail("sizes must be positive (the numbers of maps may be 0)");
    if (check_map(s->h, s->w, s->H, s->W) != MASKIOU_OK) return MASKIOU_ERR_ARGUMENT;
    if ((long long)s->F * s->h * s->w > 0x7fffffffLL)
        return err.fail("F * h * w = %lld does not fit 31 bits", (long long)s->F * s->h * s->w);
    if (entries_of(*s) > 0x7fffffffLL) return err.fail("Na * Nb + Na + Nb = %lld does not fit 31 bits", entries_of(*s));
    return MASKIOU_OK;
}

template <typename T>
int launch_pairwise(int reduce, const void *a, const void *b, const maskiou_shape &s, double eps, void *ws, void *inter,
                    void *sum_a, void *sum_b, void *iou, hipStream_t st)
{
    typedef typename Acc<T>::type A;
    const Cut c = cut_of(s);
    const int BA = (int)cdiv(s.Na, kBlock), BB = (int)cdiv(s.Nb, kBlock);
    unsigned g1, g2;
    if (err.grid_of((long long)s.F * c.splits * BA * BB, &g1) || err.grid_of(cdiv((long long)s.Na * s.Nb, kThreads), &g2))
        return MASKIOU_ERR_ARGUMENT;
    hipLaunchKernelGGL((pairwise_kernel<T>), dim3(g1), dim3(kThreads), 0, st, (const T *)a, (const T *)b, (A *)ws, s, c, BA, BB);
    hipLaunchKernelGGL((combine_kernel<A>), dim3(g2), dim3(kThreads), 0, st, (const A *)ws, (A *)inter, (A *)sum_a, (A *)sum_b,
                       (A *)iou, s, c.splits, reduce, (A)eps);
    return err.check_launch("maskiou_pairwise");
}

template <typename T>
int launch_binarize(int layout, const void *src, int N, int h, int w, int H, int W, void *out, hipStream_t st)
{
    const int tiles = (int)cdiv((long long)H * W, kBinTile);
    unsigned g1;
    if (err.grid_of((long long)N * tiles, &g1)) return MASKIOU_ERR_ARGUMENT;
    hipLaunchKernelGGL((binarize_kernel<T>), dim3(g1), dim3(kThreads), 0, st, (const T *)src, (unsigned char *)out, h, w, H, W,
                       tiles, layout == MASKIOU_COL_MAJOR ? 1 : 0);
    return err.check_launch("maskiou_binarize");
}

}  // namespace maskiou

using namespace maskiou;

extern "C" {

int maskiou_version(void) { return MASKIOU_ABI_VERSION; }

const char *maskiou_last_error(void) { return err.msg; }

int maskiou_tile(int which)
{
    switch (which) {
    case MASKIOU_TILE_BLOCK: return kBlock;
    case MASKIOU_TILE_ROWS: return kTH;
    case MASKIOU_TILE_COLS: return kTW;
    case MASKIOU_TILE_SPLIT_TILES: return kSplitTiles;
    case MASKIOU_TILE_MAX_SPLITS: return kMaxSplits;
    case MASKIOU_TILE_BIN_PIXELS: return kBinTile;
    case MASKIOU_TILE_BIN_SRC: return kBinSrc;
    default: return -1;
    }
}

long long maskiou_workspace_bytes(int dtype, const maskiou_shape *shape)
{
    err.clear();
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (check_shape(shape) != MASKIOU_OK) return MASKIOU_ERR_ARGUMENT;
    if (shape->Na == 0 || shape->Nb == 0) return 0;
    const long long bytes = (long long)shape->F * cut_of(*shape).splits * entries_of(*shape) * acc_size(dtype);
    return (bytes + 255) / 256 * 256;
}

int maskiou_pairwise(int dtype, int reduce, const void *a, const void *b, const maskiou_shape *shape, double eps,
                     void *workspace, void *inter, void *sum_a, void *sum_b, void *iou, void *stream)
{
    err.clear();
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (reduce != MASKIOU_VOLUME && reduce != MASKIOU_FRAME) return err.fail("bad reduce code %lld", reduce);
    if (check_shape(shape) != MASKIOU_OK) return MASKIOU_ERR_ARGUMENT;
    if (!(eps >= 0.0) || eps > 1.0e30) return err.fail("eps must be a finite number that is not negative");
    const maskiou_shape &s = *shape;
    if (s.Na == 0 || s.Nb == 0) return MASKIOU_OK;
    if (!a || !b || !workspace || !inter || !sum_a || !sum_b || !iou)
        return err.fail("null pointer: a, b, workspace, inter, sum_a, sum_b and iou are required");
    hipStream_t st = (hipStream_t)stream;
    return dispatch(dtype, [&](auto t) {
        return launch_pairwise<type_of<decltype(t)>>(reduce, a, b, s, eps, workspace, inter, sum_a, sum_b, iou, st);
    });
}

int maskiou_binarize(int dtype, int layout, const void *src, int N, int h, int w, int H, int W, void *out, void *stream)
{
    err.clear();
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (layout != MASKIOU_ROW_MAJOR && layout != MASKIOU_COL_MAJOR) return err.fail("bad layout code %lld", layout);
    if (N < 0) return err.fail("sizes must be positive (the numbers of maps may be 0)");
    if (check_map(h, w, H, W) != MASKIOU_OK) return MASKIOU_ERR_ARGUMENT;
    if (N == 0) return MASKIOU_OK;
    if (!src || !out) return err.fail("null pointer: src and out are required");
    hipStream_t st = (hipStream_t)stream;
    return dispatch(dtype, [&](auto t) { return launch_binarize<type_of<decltype(t)>>(layout, src, N, h, w, H, W, out, st); });
}

}  // extern "C"
