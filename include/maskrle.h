/*
 * maskrle.h -- C ABI of the run-length encoder of the clip stitching (DeVIS Tracker.process_masks / encode_mask: what the
 * COCO encoder counts before it packs its string) in libmsda_hip.so: from small logit maps straight to the run lengths of the
 * binarised full-resolution masks.  The byte map of the masks never exists in memory.
 *
 * Geometry: logit maps of (h, w) pixels, the target size (H, W), P = H*W.
 *
 * Bits: bit = x > 0 ? 1 : 0, x the resampled logit -- the rule of maskloss.h as maskiou.h states its evaluation (float for
 * MASKRLE_F32 / BF16 / F16, double for MASKRLE_F64; a tap of weight 0 contributes nothing; NaN gives 0).  The bits are those
 * of maskiou_binarize for every pixel: both units evaluate one definition of the taps.
 *
 * Runs: the mask is walked in column-major (Fortran) order, position q = x * H + y, as the COCO encoder walks it.  The
 * counts are the lengths of the maximal runs of equal bits, alternating, starting with a run of zeros, which has length 0
 * when pixel (0, 0) is set.  With t_0 < t_1 < ... < t_{T-1} the walk positions whose bit differs from its predecessor's (a
 * virtual 0 bit stands before position 0):
 *     counts = [t_0, t_1 - t_0, ..., t_{T-1} - t_{T-2}, P - t_{T-1}],   R = T + 1 of them, their sum P.
 * An all-zero mask gives [P]; an all-one mask gives [0, P].
 *
 * Row layout: runs [N, 1 + max_runs] int32, dense.
 *     runs[n, 0]                          R_n, the true number of runs, also when it exceeds max_runs
 *     runs[n, 1 : 1 + min(R_n, max_runs)] the counts, or their first max_runs
 *     the rest of the row                 0
 * Every element of runs is written and nothing outside it.  A row with R_n > max_runs is truncated: its mask has to be
 * encoded another way by the caller.
 *
 * The results are integers and depend on src[n] and (H, W) alone: a mask has the same row alone and inside any batch,
 * whatever the workspace held.  There are no atomics: a thread's first output slot comes from a scan in a fixed order.
 *
 * Conventions (those of maskiou.h)
 *   - every pointer is a DEVICE pointer; tensors are dense; src in `dtype`, which needs element alignment only; runs needs
 *     4-byte alignment;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and
 *     never synchronise (HIP-graph capture works), and are re-entrant;
 *   - element offsets are 64-bit; h*w, P and the number of workgroups of a launch must fit 31 bits, so every count fits
 *     an int32;
 *   - return value: MASKRLE_OK (0) or a negative maskrle_status; on failure maskrle_last_error() returns a thread-local
 *     message.  Arguments are checked before any HIP call, so argument errors are reported without a GPU.
 */
#ifndef MASKRLE_H
#define MASKRLE_H

#ifdef __cplusplus
extern "C" {
#endif

#define MASKRLE_ABI_VERSION 1

typedef enum maskrle_status { MASKRLE_OK = 0, MASKRLE_ERR_ARGUMENT = -1, MASKRLE_ERR_HIP = -2 } maskrle_status;

typedef enum maskrle_dtype { MASKRLE_F32 = 0, MASKRLE_F64 = 1, MASKRLE_BF16 = 2, MASKRLE_F16 = 3 } maskrle_dtype;

/* maskrle_tile(): which constant of the kernels */
#define MASKRLE_TILE_BITS_PIXELS 0  /* consecutive walk positions a workgroup of the bits pass owns, 16 per lane */
#define MASKRLE_TILE_WORD_PIXELS 1  /* walk positions per packed word of the workspace: bit b of word i is position 64*i + b */
#define MASKRLE_TILE_BITS_SRC 2     /* source elements a bits-pass workgroup keeps in LDS; a tile needing more reads memory */
#define MASKRLE_TILE_RUNS_THREADS 3 /* threads of the one workgroup that counts a mask's runs, a contiguous range of words each */

int maskrle_version(void);
const char *maskrle_last_error(void);
int maskrle_tile(int which);        /* -1 for an unknown constant */

/* Bytes of the workspace of maskrle_encode, a multiple of 256; negative on a bad argument: N * ceil(P / WORD_PIXELS) words
 * of 8 bytes; 0 when N is 0.  Host arithmetic only. */
long long maskrle_workspace_bytes(int N, int H, int W);

/* src [N, h, w] -> runs [N, 1 + max_runs] in two enqueued passes:
 *   bits  per BITS_PIXELS walk positions of a mask: the resampled logits' signs, 16 per lane, packed by four neighbouring
 *         lanes into one 64-bit word -> workspace (the bits past P of a mask's last word are 0);
 *   runs  per mask, one workgroup: per thread the transitions of a contiguous range of words (popcount of w ^ (w << 1 |
 *         carry)), an exclusive scan of those numbers and a running maximum of the last transition's position, then the
 *         thread's counts into its slots; R_n, the final count and the row's zero tail.
 * max_runs >= 1.  workspace: at least maskrle_workspace_bytes() bytes, 16-byte aligned, uninitialised.  N == 0 is a no-op. */
int maskrle_encode(int dtype, const void *src, int N, int h, int w, int H, int W, int max_runs, void *workspace, void *runs,
                   void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MASKRLE_H */
