/*
 * boxmatch.h -- C ABI of the criterion's box geometry in libmsda_hip.so: the cost matrix the
 * Hungarian matchers of DeVIS hand to the assignment solver (DeVISHungarianMatcher.forward and HungarianMatcher.forward with
 * focal_loss), and the two box losses of matched pairs (SetCriterion.loss_boxes), forward and backward.  Both are built on
 * one definition of the generalized IoU of two boxes.
 *
 * Boxes are (cx, cy, w, h).  Arithmetic is float for BOXMATCH_F32 / BF16 / F16 and double for BOXMATCH_F64, without
 * contraction into fused multiply-adds, one lane per result, every loop in ascending order: there are no atomics on floating
 * values, so every result is bitwise reproducible and depends on the inputs it reads alone.
 *
 * GIoU(s, t), with eps = 1e-6 exactly where the reference's box_ops.generalized_box_iou / multi_giou have it:
 *     (x0, y0, x1, y1) = (cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h)                        of s and of t
 *     inter = max(min(sx1, tx1) - max(sx0, tx0), 0) * max(min(sy1, ty1) - max(sy0, ty0), 0)
 *     union = (sx1 - sx0) * (sy1 - sy0) + (tx1 - tx0) * (ty1 - ty0) - inter
 *     area  = max(max(sx1, tx1) - min(sx0, tx0), 0) * max(max(sy1, ty1) - min(sy0, ty0), 0)
 *     GIoU  = (inter + eps) / (union + eps) - ((area - union) + eps) / (area + eps)
 * Its derivative with respect to s is the one torch's autograd gives for that composition, also where it is not smooth:
 *     max(a, b) and min(a, b) of equal arguments give each argument half of the gradient;
 *     max(v, 0) (clamp(min=0)) passes the gradient where v >= 0, v == 0 included;
 *     |v| has derivative 0 at v == 0 (the L1 term).
 * Identical boxes s == t meet every tie at once.
 *
 * Matching cost (boxmatch_cost).  L independent problems, F frames, R rows, T targets, C classes:
 *     logits [L, F, R, C], boxes [L, F, R, 4] in `dtype`; tgt_labels int64 [T, F]; tgt_boxes [T, F, 4] in `dtype`
 *     (BOXMATCH_TARGET_SAME) or float32 (BOXMATCH_TARGET_F32, beside a 16-bit dtype); all dense.
 *     cost[l, r, t] = cost_class * mean_f cls(logits[l, f, r, tgt_labels[t, f]])
 *                   + cost_bbox  * L1
 *                   + cost_giou  * (-mean_f GIoU(boxes[l, f, r], tgt_boxes[t, f]))
 *     cls(x) = alpha * q^2 * (-log(p + 1e-8)) - (1 - alpha) * p^2 * (-log(q + 1e-8)),  p = sigmoid(x), q = sigmoid(-x)
 *         (the reference's focal cost with its gamma 2; 1 - p is evaluated as sigmoid(-x), so the value follows the
 *         formula for every finite logit and is finite at +-inf);
 *     L1 = BOXMATCH_L1_MEAN: sum over f and the 4 coordinates of |box - tgt| / (4 * F);
 *          BOXMATCH_L1_SUM:  the same sum / F.
 *   cost [L, R, T] is in the arithmetic type.  One launch of one lane per entry, no workspace; only the T * F logits of a row
 *   are read.  An entry is its lane's loop over f = 0 .. F-1: it has the same bits whatever else the call holds.
 *   status int32 [3], zeroed by the call on `stream` and then counted with integer atomic adds, each item once:
 *     [0] prediction boxes (l, f, r) with x1 < x0 or y1 < y0;   [1] the same for the target boxes (t, f);
 *     [2] labels outside [0, C).
 *   A label outside [0, C) is never used as an index: the entries of its target are NaN.  A NaN input gives NaN in the
 *   entries that read it and nowhere else.  L * R * T == 0 is a no-op that dereferences and writes nothing, status included.
 *
 * Box losses (boxmatch_loss_forward / boxmatch_loss_backward).  src [N, 4] in `dtype`, target [N, 4] as tgt_boxes above:
 *     l1[n] = sum over the 4 coordinates of |src[n] - target[n]|,   giou[n] = 1 - GIoU(src[n], target[n])
 *     grad_src[n] = grad_l1[n] * sign(src[n] - target[n]) - grad_giou[n] * dGIoU / dsrc[n]
 *   l1, giou, grad_l1, grad_giou [N] are in the arithmetic type, grad_src [N, 4] in `dtype`.  One launch of one lane per row
 *   each.  N == 0 is a no-op.
 *
 * Conventions (those of maskloss.h)
 *   - every pointer is a DEVICE pointer; tensors are dense and need element alignment only;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and never
 *     synchronise (HIP-graph capture works), and are re-entrant;
 *   - element offsets are 64-bit; L * R * T, L * F * R, T * F and N must fit 31 bits;
 *   - return value: BOXMATCH_OK (0) or a negative boxmatch_status; on failure boxmatch_last_error() returns a thread-local
 *     message.  Arguments are checked before any HIP call, so argument errors are reported without a GPU.
 */
#ifndef BOXMATCH_H
#define BOXMATCH_H

#ifdef __cplusplus
extern "C" {
#endif

#define BOXMATCH_ABI_VERSION 1

typedef enum boxmatch_status { BOXMATCH_OK = 0, BOXMATCH_ERR_ARGUMENT = -1, BOXMATCH_ERR_HIP = -2 } boxmatch_status;

typedef enum boxmatch_dtype { BOXMATCH_F32 = 0, BOXMATCH_F64 = 1, BOXMATCH_BF16 = 2, BOXMATCH_F16 = 3 } boxmatch_dtype;

typedef enum boxmatch_target { BOXMATCH_TARGET_SAME = 0, BOXMATCH_TARGET_F32 = 1 } boxmatch_target;

typedef enum boxmatch_l1 { BOXMATCH_L1_MEAN = 0, BOXMATCH_L1_SUM = 1 } boxmatch_l1;

typedef struct boxmatch_shape {
    int L, F, R, T, C;      /* problems, frames, rows, targets, classes */
} boxmatch_shape;

int boxmatch_version(void);
const char *boxmatch_last_error(void);

int boxmatch_cost(int dtype, int target, const void *logits, const void *boxes, const long long *tgt_labels,
                  const void *tgt_boxes, const boxmatch_shape *shape, double cost_class, double cost_bbox, double cost_giou,
                  int l1, double alpha, void *cost, int *status, void *stream);

int boxmatch_loss_forward(int dtype, int target, const void *src, const void *tgt, int N, void *l1, void *giou, void *stream);

int boxmatch_loss_backward(int dtype, int target, const void *src, const void *tgt, const void *grad_l1, const void *grad_giou,
                           int N, void *grad_src, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BOXMATCH_H */
