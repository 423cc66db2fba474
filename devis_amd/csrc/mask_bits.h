// mask_bits.h -- the bits pass of the clip-stitching units that work on packed masks (maskrle.hip: the run-length encoder;
// maskbiou.hip: the binary mask IoU): from small logit maps to the signs of the resampled logits along the column-major
// walk, 64 walk positions to a word.  One definition, included by both units, on the tap rule of mask_taps.h, so that the
// bits of both are those of maskiou_binarize by construction.  The kernel has internal linkage: each unit carries and
// registers an instantiation of its own.
#ifndef MASK_BITS_H_
#define MASK_BITS_H_
#include "op_common.h"       // (fp contraction off)
#include "mask_taps.h"

namespace devis {
namespace {

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

__host__ __device__ inline int words_of(int P) { return (int)(((long long)P + kWordBits - 1) / kWordBits); }

// ---- bits -------------------------------------------------------------------------------------------------------------
// The column-major walk of maskiou.hip's binarize_kernel: a workgroup owns kBitsTile consecutive walk positions q = x * H + y
// of one mask, a lane kPer of them.  The tile is a few destination columns, so its taps touch a few source columns: they are
// staged in LDS in the arithmetic type, as [source column][source row], when they fit kBitsSrc elements, else read from
// memory (the same expression on the same values either way).  A lane packs its signs into 16 bits; lanes 4k .. 4k+3 of a
// wave combine theirs into the word of positions 64 * (tile * kBitsWords + tid / 4) ..., which lane 4k stores.  Lanes past
// the mask's end contribute zeros, so the bits past P of the last word are 0; words past the mask's last are not written.
// Mask n's words are ws[n * words_of(P) ...].
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

}  // namespace
}  // namespace devis
#endif  // MASK_BITS_H_
