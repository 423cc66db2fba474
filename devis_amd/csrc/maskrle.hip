// maskrle.hip -- the run-length encoder of the clip stitching (include/maskrle.h): from small logit maps
// to the COCO run lengths of the binarised full-resolution masks in two passes -- the bits of the column-major walk, packed 64
// to a word, then per mask the transitions of those words, counted, scanned and written as differences of positions.  Neither
// the byte map nor anything else of H*W bytes is written.  gfx950, wave64, plain HIP; integers only after the sign of the
// resampled logit, no atomics: a thread's output slots come from a scan in a fixed order.
//
// The bits pass is csrc/mask_bits.h, a template of the storage type of the logits alone.
#include "op_common.h"       // (fp contraction off)
#include "mask_taps.h"
#include "mask_bits.h"      // bits_kernel, its constants and words_of: shared with maskbiou.hip
#include "maskrle.h"

namespace maskrle {

using namespace devis;

static_assert(MASKRLE_OK == kOk && MASKRLE_ERR_ARGUMENT == kErrArgument && MASKRLE_ERR_HIP == kErrHip, "status codes");
static_assert(MASKRLE_F32 == kF32 && MASKRLE_F64 == kF64 && MASKRLE_BF16 == kBF16 && MASKRLE_F16 == kF16, "dtype codes");

thread_local Status err;     // maskrle_last_error()

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
