// maskbiou.hip -- the binary mask IoU of the clip stitching (include/maskbiou.h): from two sets of small
// logit maps to the pixel counts of the binarised full-resolution masks -- per pair and frame the intersection, per map its
// area -- in two passes: the bits of the column-major walk, packed 64 to a word (csrc/mask_bits.h, the pass of maskrle.hip),
// then a blocked "binary product" of the two sets of words, popcount(a & b) in place of a multiply-add.  gfx950, wave64,
// plain HIP; integers only after the sign of the resampled logit.
#include "op_common.h"       // (fp contraction off)
#include "mask_bits.h"
#include "maskbiou.h"

namespace maskbiou {

using namespace devis;

static_assert(MASKBIOU_OK == kOk && MASKBIOU_ERR_ARGUMENT == kErrArgument && MASKBIOU_ERR_HIP == kErrHip, "status codes");
static_assert(MASKBIOU_F32 == kF32 && MASKBIOU_F64 == kF64 && MASKBIOU_BF16 == kBF16 && MASKBIOU_F16 == kF16, "dtype codes");

constexpr int kBlock = 32;                      // pairs pass: a workgroup owns kBlock x kBlock pairs
constexpr int kSide = 16;                       // ... as kSide x kSide threads of a 2 x 2 register tile each
constexpr int kChunk = 32;                      // words of each operand row staged in LDS at a time
constexpr int kSplit = 256;                     // words of a mask per workgroup
constexpr int kPitch = kBlock + 1;              // words between two chunk positions of the LDS tiles (see pairs_kernel)
static_assert(kSide * kSide == kThreads && 2 * kSide == kBlock && kSplit % kChunk == 0, "tile shape");
static_assert(2 * kBlock * kChunk % kThreads == 0 && kThreads % kChunk == 0, "the staging loop covers both tiles evenly");
static_assert(2 * kBlock <= 64, "one wave counts the areas, a lane per operand row");

thread_local Status err;     // maskbiou_last_error()

// ---- zero -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void zero_kernel(int *__restrict__ inter, int *__restrict__ area_a, int *__restrict__ area_b,
                                                        const long long n_inter, const long long n_a, const long long n_b)
{
    const long long step = (long long)gridDim.x * kThreads;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n_inter + n_a + n_b; i += step) {
        if (i < n_inter) inter[i] = 0;
        else if (i < n_inter + n_a) area_a[i - n_inter] = 0;
        else area_b[i - n_inter - n_a] = 0;
    }
}

// ---- pairs ------------------------------------------------------------------------------------------------------------
// Workgroup (split, f, bi, bj), the pair block fastest so that neighbours share operand rows in L2 and their atomics go to
// different addresses: rows i = bi * kBlock ... of a, j = bj * kBlock ... of b, frame f, words [split * kSplit, + kSplit) of
// the masks.  Per chunk of kChunk words both operands' rows go to LDS as [word of the chunk][row] with a pitch of kBlock + 1
// words; rows past Na / Nb and words past the mask's last are staged as 0.  Banks (ds_read_b64: dword (addr / 4) % 64 in
// 32-lane halves; ds_write_b64: % 32 in groups of 16 lanes):
//   - staging: 16 neighbouring lanes hold 16 consecutive words of one row, LDS words 33 * c + row: dwords 66 * c (+1), that is
//     2 * c (+1) mod 32 for c = c0 .. c0 + 15 -- 32 different banks, no conflict.  (A pitch of 32 would put them all on one.)
//   - pairs loop: thread (ty, tx) = (tid / 16, tid % 16) reads a rows ty, ty + 16 and b rows tx, tx + 16 of word c.  A half
//     wave is two values of ty (two neighbouring LDS words, broadcast to 16 lanes each) and all 16 of tx (16 consecutive LDS
//     words = 32 consecutive dwords of the 64 banks): no conflict in either read.  The layout [row][word of the chunk] with
//     a pitch of kChunk = 32 words = 64 dwords would put the 16 b rows on ONE pair of banks: 16-way.
// Areas: in block column 0 lane r < 32 of wave 0 counts the bits of a row r of the staged chunk, in block row 0 lane 32 + r
// those of b row r (consecutive LDS words: no conflict), so every map's words are counted by exactly one workgroup per
// split.  All sums are int32: a count is at most P < 2^31.
__global__ __launch_bounds__(kThreads) void pairs_kernel(const Word *__restrict__ wa, const Word *__restrict__ wb,
                                                         int *__restrict__ inter, int *__restrict__ area_a,
                                                         int *__restrict__ area_b, const int Na, const int Nb, const int F,
                                                         const int nwords, const int nbi, const int nbj)
{
    __shared__ Word sa[kChunk * kPitch], sb[kChunk * kPitch];
    const int tid = threadIdx.x, tx = tid % kSide, ty = tid / kSide;
    unsigned int id = blockIdx.x;
    const int bj = id % nbj;
    id /= nbj;
    const int bi = id % nbi;
    id /= nbi;
    const int f = id % F, split = id / F;
    const int i0 = bi * kBlock, j0 = bj * kBlock;
    const int w0 = split * kSplit, w1 = nwords - w0 < kSplit ? nwords : w0 + kSplit;

    // staging: thread -> (row of the two tiles, word of the chunk), the word fastest
    const int sc = tid % kChunk, sr = tid / kChunk;
    constexpr int kRowsPerStep = kThreads / kChunk, kSteps = 2 * kBlock / kRowsPerStep;
    // areas: the operand row of lane tid of wave 0, or none
    const bool count_a = tid < kBlock && bj == 0, count_b = tid >= kBlock && tid < 2 * kBlock && bi == 0;
    const Word *counted = count_a ? sa + tid : count_b ? sb + (tid - kBlock) : sa;      // (sa: never read)
    int area = 0;

    int acc00 = 0, acc01 = 0, acc10 = 0, acc11 = 0;
    for (int c0 = w0; c0 < w1; c0 += kChunk) {
        if (c0 != w0) __syncthreads();                  // the previous chunk has been read
#pragma unroll
        for (int s = 0; s < kSteps; ++s) {
            const int r = s * kRowsPerStep + sr;        // 0 .. kBlock - 1: a rows, kBlock .. 2 * kBlock - 1: b rows
            const bool is_a = r < kBlock;               // (uniform per s: kBlock is a multiple of kRowsPerStep)
            const int row = is_a ? i0 + r : j0 + r - kBlock, rows = is_a ? Na : Nb;
            Word v = 0ull;
            if (row < rows && c0 + sc < w1) v = (is_a ? wa : wb)[((long long)row * F + f) * nwords + c0 + sc];
            (is_a ? sa : sb)[sc * kPitch + (is_a ? r : r - kBlock)] = v;
        }
        __syncthreads();
        if (count_a || count_b) {
#pragma unroll 8
            for (int c = 0; c < kChunk; ++c) area += __popcll(counted[c * kPitch]);
        }
#pragma unroll 8
        for (int c = 0; c < kChunk; ++c) {
            const Word a0 = sa[c * kPitch + ty], a1 = sa[c * kPitch + ty + kSide];
            const Word b0 = sb[c * kPitch + tx], b1 = sb[c * kPitch + tx + kSide];
            acc00 += __popcll(a0 & b0);
            acc01 += __popcll(a0 & b1);
            acc10 += __popcll(a1 & b0);
            acc11 += __popcll(a1 & b1);
        }
    }
    const int ia = i0 + ty, ib = ia + kSide, ja = j0 + tx, jb = ja + kSide;
    if (ia < Na && ja < Nb) atomicAdd(inter + ((long long)ia * Nb + ja) * F + f, acc00);
    if (ia < Na && jb < Nb) atomicAdd(inter + ((long long)ia * Nb + jb) * F + f, acc01);
    if (ib < Na && ja < Nb) atomicAdd(inter + ((long long)ib * Nb + ja) * F + f, acc10);
    if (ib < Na && jb < Nb) atomicAdd(inter + ((long long)ib * Nb + jb) * F + f, acc11);
    if (count_a && i0 + tid < Na) atomicAdd(area_a + (long long)(i0 + tid) * F + f, area);
    if (count_b && j0 + tid - kBlock < Nb) atomicAdd(area_b + (long long)(j0 + tid - kBlock) * F + f, area);
}

// ---- host -----------------------------------------------------------------------------------------------------------
int check_target(int Na, int Nb, int F, int H, int W)
{
    if (Na < 0 || Nb < 0 || F < 1 || H <= 0 || W <= 0) return err.fail("sizes must be positive (the number of maps of a side may be 0)");
    if ((long long)H * W > 0x7fffffffLL) return err.fail("H * W = %lld does not fit 31 bits", (long long)H * W);
    if (((long long)Na + Nb) * F > 0x7fffffffLL) return err.fail("(Na + Nb) * F = %lld does not fit 31 bits", ((long long)Na + Nb) * F);
    // (Na * Nb < 2^62, and the product with F is only formed when that is below 2^31)
    if ((long long)Na * Nb > 0x7fffffffLL || (long long)Na * Nb * F > 0x7fffffffLL)
        return err.fail("Na * Nb * F does not fit 31 bits (Na * Nb = %lld, F = %lld)", (long long)Na * Nb, F);
    return MASKBIOU_OK;
}

template <typename T>
int launch_counts(const void *a, const void *b, int Na, int Nb, int F, int h, int w, int H, int W, void *ws, void *inter,
                  void *area_a, void *area_b, hipStream_t st)
{
    const int P = H * W, nwords = words_of(P), tiles = (int)cdiv(P, kBitsTile);
    const int nbi = (int)cdiv(Na, kBlock), nbj = (int)cdiv(Nb, kBlock), splits = (int)cdiv(nwords, kSplit);
    const long long n_inter = (long long)Na * Nb * F, n_a = (long long)Na * F, n_b = (long long)Nb * F;
    unsigned g0, ga, gb, gp;
    if (err.grid_of(cdiv(n_inter + n_a + n_b, kThreads), &g0) || err.grid_of(n_a * tiles, &ga) || err.grid_of(n_b * tiles, &gb) ||
        err.grid_of((long long)splits * F * nbi * nbj, &gp))
        return MASKBIOU_ERR_ARGUMENT;
    Word *wa = (Word *)ws, *wb = wa + n_a * nwords;
    hipLaunchKernelGGL(zero_kernel, dim3(g0 < 4096u ? g0 : 4096u), dim3(kThreads), 0, st, (int *)inter, (int *)area_a, (int *)area_b,
                       n_inter, n_a, n_b);
    hipLaunchKernelGGL((bits_kernel<T>), dim3(ga), dim3(kThreads), 0, st, (const T *)a, wa, h, w, H, W, tiles);
    hipLaunchKernelGGL((bits_kernel<T>), dim3(gb), dim3(kThreads), 0, st, (const T *)b, wb, h, w, H, W, tiles);
    hipLaunchKernelGGL(pairs_kernel, dim3(gp), dim3(kThreads), 0, st, (const Word *)wa, (const Word *)wb, (int *)inter,
                       (int *)area_a, (int *)area_b, Na, Nb, F, nwords, nbi, nbj);
    return err.check_launch("maskbiou_counts");
}

}  // namespace maskbiou

using namespace maskbiou;

extern "C" {

int maskbiou_version(void) { return MASKBIOU_ABI_VERSION; }

const char *maskbiou_last_error(void) { return err.msg; }

int maskbiou_tile(int which)
{
    switch (which) {
    case MASKBIOU_TILE_BLOCK: return kBlock;
    case MASKBIOU_TILE_CHUNK_WORDS: return kChunk;
    case MASKBIOU_TILE_SPLIT_WORDS: return kSplit;
    default: return -1;
    }
}

long long maskbiou_workspace_bytes(int Na, int Nb, int F, int H, int W)
{
    err.clear();
    if (check_target(Na, Nb, F, H, W) != MASKBIOU_OK) return MASKBIOU_ERR_ARGUMENT;
    if (Na == 0 || Nb == 0) return 0;
    const long long bytes = ((long long)Na + Nb) * F * words_of(H * W) * (long long)sizeof(Word);
    return (bytes + 255) / 256 * 256;
}

int maskbiou_counts(int dtype, const void *a, const void *b, int Na, int Nb, int F, int h, int w, int H, int W, void *workspace,
                    void *inter, void *area_a, void *area_b, void *stream)
{
    err.clear();
    if (!elem_size(dtype)) return err.fail("bad dtype code %lld", dtype);
    if (h <= 0 || w <= 0) return err.fail("sizes must be positive (the number of maps of a side may be 0)");
    if (check_target(Na, Nb, F, H, W) != MASKBIOU_OK) return MASKBIOU_ERR_ARGUMENT;
    if ((long long)h * w > 0x7fffffffLL) return err.fail("h * w = %lld does not fit 31 bits", (long long)h * w);
    if (Na == 0 || Nb == 0) return MASKBIOU_OK;
    if (!a || !b || !workspace || !inter || !area_a || !area_b)
        return err.fail("null pointer: a, b, workspace, inter, area_a and area_b are required");
    hipStream_t st = (hipStream_t)stream;
    return dispatch(dtype, [&](auto t) {
        return launch_counts<type_of<decltype(t)>>(a, b, Na, Nb, F, h, w, H, W, workspace, inter, area_a, area_b, st);
    });
}

}  // extern "C"
