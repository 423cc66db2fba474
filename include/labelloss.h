/*
 * labelloss.h -- C ABI of the criterion's label loss in libmsda_hip.so: what DeVIS's
 * SetCriterion.loss_labels_focal computes -- the target class of every query from the matcher's indices, the sigmoid focal
 * loss of all logits against those classes, and the matched queries' top-1 count behind class_error -- as one operator,
 * forward and backward.  No one-hot tensor, no boolean-mask indexing, nothing read on the host.
 *
 * Geometry: logits [R, C] in `dtype`, R = B * N rows flattened by the caller, C classes.  M matches: rows int64 [M] (the row
 * index b * N + src), labels int64 [M], valid uint8 / bool [M] (nonzero is valid) or NULL for all valid.
 *
 * Definition
 *   A match m is GOOD when it is valid, 0 <= rows[m] < R and 0 <= labels[m] <= C.  The label C is the reference's "no
 *   object" column: a good match with no positive.  Matches that are not good are ignored, except by counts[2] / counts[3].
 *   target_classes[r] (int32 [R], an output) is the label of the good match with the HIGHEST m among those with
 *   rows[m] == r, and C if there is none: the CPU's last-write-wins rule of index_put_ (the reference never produces
 *   duplicates, so this only fixes a rule where it had none).
 *   t[r, c] = (c == target_classes[r]).
 *
 *   Per element, with x the logit, e = exp(-|x|) and the expressions of maskloss.h at gamma = 2:
 *     p     = sigmoid(x)  = x >= 0 ? 1/(1+e) : e/(1+e)
 *     1 - p = sigmoid(-x) = x >= 0 ? e/(1+e) : 1/(1+e)          (as boxmatch.h evaluates it: no cancellation)
 *     ce    = max(x,0) - x*t + log1p(e), the subtraction evaluated for t = 1 as max(-x,0) + log1p(e): the same bits for
 *             every finite x, and 0 instead of inf - inf at x = +inf
 *     m     = t ? 1-p : p
 *     focal = ce * m * m         and, if alpha >= 0, focal *= (t ? alpha : 1 - alpha); alpha < 0 means unweighted
 *   focal_sum [1], in the arithmetic type, is the sum over all R * C elements.  At x = +-inf an element gives what these
 *   expressions give (inf or 0); a NaN logit makes focal_sum NaN.
 *
 *   counts int32 [4]:
 *     [0] good matches (every duplicate counts);
 *     [1] good matches whose row's argmax over c equals labels[m].  The LOWEST class index wins a tie, and a row that
 *         contains a NaN is never correct (torch.topk promises neither).  A label C is never correct;
 *     [2] valid matches with a row outside [0, R);
 *     [3] valid matches with a label outside [0, C].
 *
 *   Backward, with x, p, 1-p, ce, m recomputed by the forward's expressions and alpha_t = (t ? alpha : 1 - alpha) or 1:
 *     grad_logits[r, c] = grad_sum[0] * alpha_t * ((p - t) * m*m + ce * 2*m * (1 - 2*t) * p*(1-p))
 *   with p - t evaluated for t = 1 as -(1-p), again without the cancellation, and written in `dtype`.  grad_sum [1] is a DEVICE pointer in the arithmetic type; it is never read on the host.  A NaN logit
 *   makes its own element of grad_logits NaN and no other.
 *
 * Arithmetic is float for LABELLOSS_F32 / BF16 / F16 and double for LABELLOSS_F64, every product and sum rounded on its own
 * (no fused multiply-add).  There are no atomics on memory and nothing is zeroed: every output word is written by the call.
 * The summation order is fixed -- a lane adds its elements ascending, lanes are combined by butterflies, waves and tiles
 * ascending -- and depends on (R, C) alone: focal_sum is bitwise reproducible and does not depend on the order of the
 * matches; target_classes and grad_logits of a row depend on that row's logits and matches alone.
 *
 * Kernels.  The operator is bound by launch latency (the criterion has R * C = 12 000 logits), so what counts is the number
 * of launches, no temporaries and the fixed order:
 *   forward   a tiles pass and a combine.  A workgroup owns a tile of whole rows, a contiguous range of logits of at most
 *             labelloss_tile(LABELLOSS_TILE_ELEMENTS) elements (a longer row is one tile).  It sets an LDS table of its rows
 *             to "none", walks ALL M matches strided over its lanes and keeps, by an LDS integer atomicMax on m, the good
 *             ones whose row is its own; writes target_classes of its rows; sums the focal terms; finds, one wave per match
 *             with lanes strided over C, the argmax of each good match of its rows; and writes one record (the focal partial
 *             and the four counts) to the workspace.  counts[2] and counts[3] are counted by workgroup 0.  The combine pass,
 *             one workgroup, adds the records -- lanes strided over the tiles ascending, then butterflies, then waves
 *             ascending -- and writes focal_sum and counts.  A call of one tile writes its results directly: one launch.
 *             Every workgroup scanning all M matches is deliberate: at the criterion's shapes M is at most a few hundred
 *             and there is a handful of tiles, so a pass that bins the matches first would cost a launch to save nothing.
 *   backward  one elementwise launch over R * C that reads logits, target_classes and grad_sum[0]; no LDS, no workspace.
 *
 * Conventions (those of boxmatch.h / maskloss.h)
 *   - every pointer is a DEVICE pointer; tensors are dense and need element alignment only;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and never
 *     synchronise (HIP-graph capture works), and are re-entrant;
 *   - element offsets are 64-bit; R * C and M must fit 31 bits;
 *   - return value: LABELLOSS_OK (0) or a negative labelloss_status; on failure labelloss_last_error() returns a
 *     thread-local message.  Arguments are checked before any HIP call, so argument errors are reported without a GPU.
 */
#ifndef LABELLOSS_H
#define LABELLOSS_H

#ifdef __cplusplus
extern "C" {
#endif

#define LABELLOSS_ABI_VERSION 1

typedef enum labelloss_status { LABELLOSS_OK = 0, LABELLOSS_ERR_ARGUMENT = -1, LABELLOSS_ERR_HIP = -2 } labelloss_status;

typedef enum labelloss_dtype { LABELLOSS_F32 = 0, LABELLOSS_F64 = 1, LABELLOSS_BF16 = 2, LABELLOSS_F16 = 3 } labelloss_dtype;

/* labelloss_tile(): which constant of the kernels' tiling */
#define LABELLOSS_TILE_ELEMENTS 0   /* logits (whole rows, consecutive) per workgroup of the forward pass, at most */

typedef struct labelloss_shape {
    int R, C, M;            /* rows, classes, matches */
} labelloss_shape;

int labelloss_version(void);
const char *labelloss_last_error(void);
int labelloss_tile(int which);      /* -1 for an unknown constant */

/* Bytes of the workspace of labelloss_forward, a multiple of 256; negative on a bad argument: one record of 32 bytes per
 * tile, or 0 when the call is one tile.  The backward needs none.  Host arithmetic only. */
long long labelloss_workspace_bytes(int dtype, const labelloss_shape *shape);

/* target_classes [R], focal_sum [1] and counts [4], every word written, in one or two enqueued passes (above).
 * workspace: at least labelloss_workspace_bytes() bytes, 16-byte aligned, uninitialised (may be NULL when that is 0).
 * R * C == 0 is a no-op that dereferences and writes nothing.  M == 0 is a normal call in which every row is background
 * (rows, labels and valid may be NULL). */
int labelloss_forward(int dtype, const void *logits, const long long *rows, const long long *labels,
                      const unsigned char *valid, const labelloss_shape *shape, double alpha, void *workspace,
                      int *target_classes, void *focal_sum, int *counts, void *stream);

/* grad_logits [R, C], every element written, in one enqueued pass.  Only R and C of `shape` are read.  R * C == 0 is a
 * no-op. */
int labelloss_backward(int dtype, const void *logits, const int *target_classes, const void *grad_sum,
                       const labelloss_shape *shape, double alpha, void *grad_logits, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LABELLOSS_H */
