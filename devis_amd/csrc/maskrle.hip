// maskrle.hip -- the run-length encoder of the clip stitching (include/maskrle.h): from small logit maps
// to the COCO run lengths of the binarised full-resolution masks in two passes -- the bits of the column-major walk, packed 64
// to a word, then per mask the transitions of those words, counted, scanned and written as differences of positions.  Neither
// the byte map nor anything else of H*W bytes is written.  gfx950, wave64, plain HIP; integers only after the sign of the
// resampled logit, no atomics: a thread's output slots come from a scan in a fixed order.
//
// The kernels are templates of the storage type of the logits alone.
#include "op_common.h"       // (fp contraction off)
#include "mask_taps.h"
#include "maskrle.h"

namespace maskrle {

using namespace devis;

static_assert(MASKRLE_OK == kOk && MASKRLE_ERR_ARGUMENT == kErrArgument && MASKRLE_ERR_HIP == kErrHip, "status codes");
static_assert(MASKRLE_F32 == kF32 && MASKRLE_F64 == kF64 && MASKRLE_BF16 == kBF16 && MASKRLE_F16 == kF16, "dtype codes");

typedef unsigned long long Word;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = 16;                        // bits pass: consecutive walk positions per lane
constexpr int kWordBits = 64;                   // walk positions per packed word
constexpr int kLanesPerWord = kWordBits / kPer; // neighbouring lanes that share a word
constexpr int kBitsTile = kThreads * kPer;      // walk positions per workgroup of the bits pass
constexpr int kBitsWords = kBitsTile / kWordBits;
constexpr int kBitsSrc = 4096;                  // bits pass: source elements kept in LDS
static_assert(kLanesPerWord == 4 && kBitsTile % kWordBits == 0, "a word is four neighbouring lanes of one wave; tiles start on words");

thread_local Status err;     // maskrle_last_error()

__host__ __device__ inline int words_of(int P) { return (int)(((long long)P + kWordBits - 1) / kWordBits); }

// ---- bits -------------------------------------------------------------------------------------------------------------
// The column-major walk of maskiou.hip's binarize_kernel: a workgroup owns kBitsTile consecutive walk positions q = x * H + y
// of one mask, a lane kPer of them.  The tile is a few destination columns, so its taps touch a few source columns: they are
// staged in LDS in the arithmetic type, as [source column][source row], when they fit kBitsSrc elements, else read from
// memory (the same expression on the same values either way).  A lane packs its signs into 16 bits; lanes 4k .. 4k+3 of a
// wave combine theirs into the word of positions 64 * (tile * kBitsWords + tid / 4) ..., which lane 4k stores.  Lanes past
// the mask's end contribute zeros, so the bits past P of the last word are 0; words past the mask's last are not written.
template <typename T>
__global__ __launch_bounds__(kThreads) void bits_kernel(const T *__restrict__ src, Word *__restrict__ ws, const int h, const int w,
                                                        const int H, const int W, const int tiles)
{
    typedef typename Acc<T>::type A;
    __shared__ A cols[kBitsSrc];
    const long long n = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles, tid = threadIdx.x;
    const int P = H * W, nwords = words_of(P);
    const A scale_x = (A)w / (A)W, scale_y = (A)h / (A)H;
    const T *sp = src + n * ((long long)h * w);
    const int base = tile * kBitsTile;                  // (tile * kBitsTile < P <= 2^31 - 1)
    const int end = P - base < kBitsTile ? P : base + kBitsTile;
    // the source columns of the tile's first and last destination column
    const int s0 = tap_at<A>(base / H, w, scale_x).i0, s1 = tap_at<A>((end - 1) / H, w, scale_x).i1;
    const bool staged = (long long)(s1 - s0 + 1) * h <= kBitsSrc;
    if (staged) {
        const int nc = s1 - s0 + 1, cnt = nc * h;       // consecutive threads read consecutive source columns
        for (int i = tid; i < cnt; i += kThreads) {
            const int y = i / nc, c = i - y * nc;
            cols[c * h + y] = (A)to_acc(sp[(long long)y * w + s0 + c]);
        }
        __syncthreads();
    }
    const int q0 = base + tid * kPer;
    unsigned int bits = 0u;
    if (q0 < end) {
        int x = q0 / H, y = q0 - x * H;
        Tap<A> tx = tap_at<A>(x, w, scale_x);
        const int cnt = end - q0 < kPer ? end - q0 : kPer;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            if (j < cnt) {
                const Tap<A> ty = tap_at<A>(y, h, scale_y);
                A v;
                if (staged) {
                    const A *ca = cols + (tx.i0 - s0) * h, *cb = cols + (tx.i1 - s0) * h;
                    v = lerp_of<A>(ty, tx, ca[ty.i0], cb[ty.i0], ca[ty.i1], cb[ty.i1]);
                } else {
                    v = logit_at<T>(sp, w, ty, tx);
                }
                bits |= (v > (A)0 ? 1u : 0u) << j;
                if (++y == H) {
                    y = 0;
                    ++x;
                    if (x < W) tx = tap_at<A>(x, w, scale_x);
                }
            }
        }
    }
    // every lane of the wave takes part in the exchange, also those past the mask's end
    unsigned int lo = (tid & 1) ? bits << kPer : bits;          // a lane pair's 32 bits
    lo |= __shfl_xor(lo, 1, 64);
    const unsigned int other = __shfl_xor(lo, 2, 64);
    const int word = tile * kBitsWords + tid / kLanesPerWord;
    if ((tid & (kLanesPerWord - 1)) == 0 && word < nwords) ws[n * nwords + word] = (Word)lo | ((Word)other << 32);
}

// ---- runs -------------------------------------------------------------------------------------------------------------
// the transitions of word i of a mask: bit b is set where walk position 64 * i + b differs from its predecessor (a 0 before
// position 0); positions past P do not count
__device__ __forceinline__ Word transitions_of(const Word *__restrict__ wp, int i, int nwords, int P)
{
    const Word v = wp[i], carry = i ? wp[i - 1] >> (kWordBits - 1) : 0ull;
    Word t = v ^ ((v << 1) | carry);
    const int tail = P & (kWordBits - 1);
    if (i == nwords - 1 && tail) t &= (1ull << tail) - 1ull;
    return t;
}

// One workgroup per mask; thread k owns the words [k * per, (k + 1) * per).  First walk: the number of transitions of the
// range and the position of its last one (-1: none).  An inclusive scan over the threads -- shuffles inside a wave, the waves'
// totals through LDS in ascending order -- of the numbers (a sum) and of the positions (a maximum: they ascend with the
// thread) gives a thread its first output slot and the transition before its range.  Second walk: transition k at position
// t_k is count k = t_k - t_{k-1} (t_{-1} = 0), written when k < max_runs.  The last thread, whose scan is the mask's totals,
// writes R = T + 1 and count T = P - t_{T-1}; the workgroup writes the zeros behind.
__global__ __launch_bounds__(kThreads) void runs_kernel(const Word *__restrict__ ws, int *__restrict__ runs, const int P,
                                                        const int max_runs)
{
    __shared__ int wave_cnt[kWaves], wave_last[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nwords = words_of(P);
    const Word *wp = ws + (long long)blockIdx.x * nwords;
    int *row = runs + (long long)blockIdx.x * ((long long)max_runs + 1);
    const int per = (nwords + kThreads - 1) / kThreads;
    const long long lo64 = (long long)tid * per;
    const int i0 = lo64 < nwords ? (int)lo64 : nwords, i1 = nwords - i0 < per ? nwords : i0 + per;

    int cnt = 0, last = -1;
    for (int i = i0; i < i1; ++i) {
        const Word t = transitions_of(wp, i, nwords, P);
        if (t) {
            cnt += __popcll(t);
            last = i * kWordBits + (kWordBits - 1 - __clzll((long long)t));
        }
    }
    int scan_cnt = cnt, scan_last = last;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int c = __shfl_up(scan_cnt, d, 64), l = __shfl_up(scan_last, d, 64);
        if (lane >= d) {
            scan_cnt += c;
            scan_last = l > scan_last ? l : scan_last;
        }
    }
    if (lane == 63) {
        wave_cnt[wave] = scan_cnt;
        wave_last[wave] = scan_last;
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
        if (v < wave) {
            scan_cnt += wave_cnt[v];
            scan_last = wave_last[v] > scan_last ? wave_last[v] : scan_last;
        }
        total += wave_cnt[v];
    }

    int k = scan_cnt - cnt;                             // exclusive: this thread's first slot
    int prev = __shfl_up(scan_last, 1, 64);             // the last transition before this thread's range, or 0
    if (lane == 0) {
        prev = -1;
#pragma unroll
        for (int v = 0; v < kWaves; ++v)
            if (v < wave && wave_last[v] > prev) prev = wave_last[v];
    }
    if (prev < 0) prev = 0;
    for (int i = i0; i < i1 && k < max_runs; ++i) {
        Word t = transitions_of(wp, i, nwords, P);
        while (t && k < max_runs) {
            const int pos = i * kWordBits + __ffsll((long long)t) - 1;
            t &= t - 1ull;
            row[1 + k] = pos - prev;
            prev = pos;
            ++k;
        }
    }
    if (tid == kThreads - 1) {
        row[0] = total + 1;
        if (total < max_runs) row[1 + total] = P - (scan_last < 0 ? 0 : scan_last);
    }
    for (long long z = (long long)total + 1 + tid; z < max_runs; z += kThreads) row[1 + z] = 0;
}

// ---- host -----------------------------------------------------------------------------------------------------------
int check_target(int N, int H, int W)
{
    if (N < 0 || H <= 0 || W <= 0) return err.fail("sizes must be positive (the number of maps may be 0)");
    if ((long long)H * W > 0x7fffffffLL) return err.fail("H * W = %lld does not fit 31 bits", (long long)H * W);
    return MASKRLE_OK;
}

template <typename T>
int launch_encode(const void *src, int N, int h, int w, int H, int W, int max_runs, void *ws, void *runs, hipStream_t st)
{
    const int P = H * W, tiles = (int)cdiv(P, kBitsTile);
    unsigned g1, g2;
    if (err.grid_of((long long)N * tiles, &g1) || err.grid_of(N, &g2)) return MASKRLE_ERR_ARGUMENT;
    hipLaunchKernelGGL((bits_kernel<T>), dim3(g1), dim3(kThreads), 0, st, (const T *)src, (Word *)ws, h, w, H, W, tiles);
    hipLaunchKernelGGL(runs_kernel, dim3(g2), dim3(kThreads), 0, st, (const Word *)ws, (int *)runs, P, max_runs);
    return err.check_launch("maskrle_encode");
}

}  // namespace maskrle

using namespace maskrle;

extern "C" {

int maskrle_version(void) { return MASKRLE_ABI_VERSION; }

const char *maskrle_last_error(void) { return err.msg; }

int maskrle_tile(int which)
{
    switch (which) {
    case MASKRLE_TILE_BITS_PIXELS: return kBitsTile;
    case MASKRLE_TILE_WORD_PIXELS: return kWordBits;
    case MASKRLE_TILE_BITS_SRC: return kBitsSrc;
    case MASKRLE_TILE_RUNS_THREADS: return kThreads;
    default: return -1;
    }
}

long long maskrle_workspace_bytes(int N, int H, int W)
{
    err.clear();
    if (check_target(N, H, W) != MASKRLE_OK) return MASKRLE_ERR_ARGUMENT;
    const long long bytes = (long long)N * words_of(H * W) * (long long)sizeof(Word);
    return (bytes + 255) / 256 * 256;
}

int maskrle_encode(int dtype, const void *src, int N, int h, int w, int H, int W, int max_runs, void *workspace, void *runs,
                   void *stream)
{
    err.clear();
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (h <= 0 || w <= 0) return err.fail("sizes must be positive (the number of maps may be 0)");
    if (check_target(N, H, W) != MASKRLE_OK) return MASKRLE_ERR_ARGUMENT;
    if ((long long)h * w > 0x7fffffffLL) return err.fail("h * w = %lld does not fit 31 bits", (long long)h * w);
    if (max_runs < 1) return err.fail("max_runs must be at least 1, got %lld", max_runs);
    if (N == 0) return MASKRLE_OK;
    if (!src || !workspace || !runs) return err.fail("null pointer: src, workspace and runs are required");
    hipStream_t st = (hipStream_t)stream;
    return dispatch(dtype, [&](auto t) {
        return launch_encode<type_of<decltype(t)>>(src, N, h, w, H, W, max_runs, workspace, runs, st);
    });
}

}  // extern "C"
