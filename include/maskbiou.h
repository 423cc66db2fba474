/*
 * maskbiou.h -- C ABI of the binary mask IoU of the clip stitching (DeVIS HungarianInferenceMatcher.iou over all pairs of
 * tracks, TEST.CLIP_TRACKING.USE_BINARY_MASK_IOU) in libmsda_hip.so: from two sets of small logit maps straight to the
 * pixel counts an IoU of the binarised full-resolution masks is made of.  Neither the byte maps nor
 * their encodings exist in memory: a mask is one bit per pixel in the workspace.
 *
 * Geometry: logit maps a [Na, F, h, w] and b [Nb, F, h, w] (F frames per track), the target size (H, W), P = H*W.
 *
 * Bits: bit = x > 0 ? 1 : 0, x the resampled logit -- the rule of maskloss.h as maskiou.h states its evaluation (float for
 * MASKBIOU_F32 / BF16 / F16, double for MASKBIOU_F64; a tap of weight 0 contributes nothing; NaN gives 0).  The bits are
 * those of maskiou_binarize and of maskrle_encode for every pixel: the three units evaluate one definition of the taps, and
 * this unit and maskrle_encode one definition of the pass that packs them.
 *
 * Counts, all int32 and dense, with A(i, f) and B(j, f) the sets of set pixels of the binarised maps:
 *     inter  [Na, Nb, F]   |A(i, f) & B(j, f)|
 *     area_a [Na, F]       |A(i, f)|
 *     area_b [Nb, F]       |B(j, f)|
 * Every element of the three is written and nothing outside them, whatever they and the workspace held -- with one
 * exception: when Na or Nb is 0 the call is a no-op, so the areas of the side that has maps (area_b [Nb, F] when only Na is
 * 0) are NOT written; a caller that wants them calls that side against one of its own maps.  The union of a pair is
 * area_a + area_b - inter; forming a ratio is the caller's.
 *
 * The results are integers and depend on a[i], b[j] and (H, W) alone: a pair has the same counts alone and inside any
 * batch.  The ranges of words a mask is split into are combined by integer atomic adds onto outputs the call itself zeroes
 * on `stream`: integer addition is associative, so the order of arrival does not show.
 *
 * Conventions (those of maskrle.h)
 *   - every pointer is a DEVICE pointer; tensors are dense; a and b in `dtype`, which needs element alignment only; the
 *     outputs need 4-byte alignment;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and
 *     never synchronise (HIP-graph capture works), and are re-entrant;
 *   - element offsets are 64-bit; h*w, P, (Na + Nb) * F, Na * Nb * F and the number of workgroups of a launch must fit 31
 *     bits, so every count fits an int32;
 *   - return value: MASKBIOU_OK (0) or a negative maskbiou_status; on failure maskbiou_last_error() returns a thread-local
 *     message.  Arguments are checked before any HIP call, so argument errors are reported without a GPU.
 */
#ifndef MASKBIOU_H
#define MASKBIOU_H

#ifdef __cplusplus
extern "C" {
#endif

#define MASKBIOU_ABI_VERSION 1

typedef enum maskbiou_status { MASKBIOU_OK = 0, MASKBIOU_ERR_ARGUMENT = -1, MASKBIOU_ERR_HIP = -2 } maskbiou_status;

typedef enum maskbiou_dtype { MASKBIOU_F32 = 0, MASKBIOU_F64 = 1, MASKBIOU_BF16 = 2, MASKBIOU_F16 = 3 } maskbiou_dtype;

/* maskbiou_tile(): which constant of the kernels */
#define MASKBIOU_TILE_BLOCK 0        /* edge of the block of (i, j) pairs a workgroup of the pair pass owns */
#define MASKBIOU_TILE_CHUNK_WORDS 1  /* 64-pixel words of each operand row a workgroup stages in LDS at a time */
#define MASKBIOU_TILE_SPLIT_WORDS 2  /* words of a mask per workgroup: a mask of more is split over several, combined by atomic adds */

int maskbiou_version(void);
const char *maskbiou_last_error(void);
int maskbiou_tile(int which);        /* -1 for an unknown constant */

/* Bytes of the workspace of maskbiou_counts, a multiple of 256; negative on a bad argument: (Na + Nb) * F * ceil(P / 64)
 * words of 8 bytes; 0 when Na or Nb is 0.  Host arithmetic only. */
long long maskbiou_workspace_bytes(int Na, int Nb, int F, int H, int W);

/* a [Na, F, h, w], b [Nb, F, h, w] -> inter [Na, Nb, F], area_a [Na, F], area_b [Nb, F] in enqueued passes:
 *   zero   the three outputs;
 *   bits   the (Na + Nb) * F maps -> workspace, by the bits pass of maskrle_encode (one launch per operand);
 *   pairs  a workgroup owns BLOCK x BLOCK pairs, one frame and SPLIT_WORDS words; per CHUNK_WORDS words it stages both
 *          operands' rows in LDS and every thread adds popcount(a & b) into a 2 x 2 register tile of pairs; the workgroups
 *          of block column 0 / block row 0 also count their a / b rows' own bits; atomic adds onto the outputs.
 * F >= 1.  workspace: at least maskbiou_workspace_bytes() bytes, 16-byte aligned, uninitialised.  Na == 0 or Nb == 0 is a
 * no-op that dereferences nothing and writes nothing, the other side's areas included (see above). */
int maskbiou_counts(int dtype, const void *a, const void *b, int Na, int Nb, int F, int h, int w, int H, int W, void *workspace,
                    void *inter, void *area_a, void *area_b, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MASKBIOU_H */
