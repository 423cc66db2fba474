/*
 * maskloss.h -- C ABI of the mask loss (DeVIS SetCriterion.loss_masks) in libmsda_hip.so: bilinear resampling of the mask
 * head's small logit maps to the target resolution, the sigmoid focal loss and the dice loss, fused into one pass over the
 * target pixels that writes per-tile partial sums and a fixed-order combine; and the backward, which gathers the
 * per-pixel derivative over each source pixel's footprint.  Nothing of the target's resolution is
 * ever written to memory.
 *
 * Geometry: src [N, h, w] logits, target [N, H, W], p = h*w, P = H*W.
 *
 * The resampled logit is PyTorch's mode="bilinear", align_corners=False rule with size= given, per axis (rows: h, H, d
 * the destination row; columns: w, W), evaluated in float32 for every dtype except float64:
 *
 *   scale = (float)h / (float)H
 *   r  = max(scale * (d + 0.5f) - 0.5f, 0)
 *   i0 = (int)r
 *   i1 = i0 + (i0 < h-1 ? 1 : 0)
 *   l1 = r - i0
 *   l0 = 1 - l1
 *   x[n,d] = l0y*(l0x*src[i0y,i0x] + l1x*src[i0y,i1x]) + l1y*(l0x*src[i1y,i0x] + l1x*src[i1y,i1x])
 *
 * every product and sum rounded on its own (no fused multiply-add).  H < h (downsampling) and H == h (the identity: l1 is
 * 0) follow the same rule.  The arithmetic type is float for MASKLOSS_F32 / BF16 / F16 and double for MASKLOSS_F64; x is
 * never rounded to a 16-bit type.
 *
 * Per pixel, with t the target value (MASKLOSS_TARGET_U8: nonzero -> 1; floating: as it is) and e = exp(-|x|):
 *   p     = sigmoid(x)              = x >= 0 ? 1/(1+e) : e/(1+e)
 *   ce    = max(x,0) - x*t + log1p(e)
 *   p_t   = p*t + (1-p)*(1-t)       m = 1 - p_t
 *   focal = ce * m^gamma            and, if alpha >= 0, focal *= alpha*t + (1-alpha)*(1-t)
 * gamma == 2 is a square, gamma == 1 is m, gamma == 0 is 1 (also at m == 0); any other gamma > 1 goes through pow.
 * 0 < gamma < 1 (an unbounded derivative at m == 0) and gamma < 0 are argument errors.
 *
 * Per instance:
 *   focal[n] = (sum over d of focal) / P
 *   A = sum p*t, B = sum p, Cn = sum t          sums[n] = (A, B, Cn)
 *   dice[n]  = 1 - (2A+1) / (B+Cn+1)
 *
 * Backward: for grad_focal [N], grad_dice [N], with x, p, ce, m recomputed by the forward's expressions,
 *   dfocal/dx = alpha_t * ((p-t) * m^gamma + ce * gamma*m^(gamma-1) * (1-2t) * p*(1-p))
 *   ddice/dx  = -(2*t*(B+Cn+1) - (2A+1)) / (B+Cn+1)^2 * p*(1-p)
 *   g[n,d]    = grad_focal[n]/P * dfocal/dx + grad_dice[n] * ddice/dx
 *   grad_src[n,s] = sum over the destination pixels d whose taps contain s of (the tap weight of s at d) * g[n,d]
 * The d of a source row (column) are a contiguous range; the sum runs rows ascending, and within a row columns ascending
 * (row sums are formed first, then weighted by the row's tap weight).  target has no gradient.
 *
 * There are no float atomics anywhere: a lane sums its pixels in ascending order, lanes are combined by butterflies, waves
 * and tiles in ascending order.  Every result is bitwise reproducible, and an instance has the same bits alone and in a
 * batch.  The order does not depend on the target kind nor on whether the target is read by vector or scalar loads.
 *
 * Conventions (those of mhstage.h)
 *   - every pointer is a DEVICE pointer unless stated; tensors are dense: src, grad_src [N, h, w] in `dtype`;
 *     target [N, H, W] in the type `target_kind` names; focal, dice, grad_focal, grad_dice [N] and sums [N, 3] in the
 *     arithmetic type;
 *   - target needs no alignment.  MASKLOSS_TARGET_U8 is read 16 pixels per lane where a lane's 16 pixels start at a
 *     16-byte aligned address (always, when target is 16-byte aligned and P is a multiple of 16), one by one otherwise;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and
 *     never synchronise (HIP-graph capture works), and are re-entrant;
 *   - element offsets are 64-bit; p, P, and the number of workgroups of a launch (N * tiles) must fit 31 bits;
 *   - return value: MASKLOSS_OK (0) or a negative maskloss_status; on failure maskloss_last_error() returns a
 *     thread-local message.  Arguments are checked before any HIP call, so argument errors are reported without a GPU.
 */
#ifndef MASKLOSS_H
#define MASKLOSS_H

#ifdef __cplusplus
extern "C" {
#endif

#define MASKLOSS_ABI_VERSION 1

typedef enum maskloss_status { MASKLOSS_OK = 0, MASKLOSS_ERR_ARGUMENT = -1, MASKLOSS_ERR_HIP = -2 } maskloss_status;

typedef enum maskloss_dtype { MASKLOSS_F32 = 0, MASKLOSS_F64 = 1, MASKLOSS_BF16 = 2, MASKLOSS_F16 = 3 } maskloss_dtype;

/* the type of target: one byte per pixel (bool, uint8), src's own dtype, or float32 */
typedef enum maskloss_target { MASKLOSS_TARGET_U8 = 0, MASKLOSS_TARGET_SAME = 1, MASKLOSS_TARGET_F32 = 2 } maskloss_target;

/* maskloss_tile(): which constant of the kernels' tiling */
#define MASKLOSS_TILE_FWD_PIXELS 0  /* destination pixels (consecutive, row-major) per workgroup of the forward pass */
#define MASKLOSS_TILE_FWD_SRC 1     /* source elements a forward workgroup keeps in LDS; a tile needing more reads memory */
#define MASKLOSS_TILE_BWD_ROWS 2    /* source rows per workgroup of the backward pass */
#define MASKLOSS_TILE_BWD_COLS 3    /* source columns per workgroup of the backward pass */
#define MASKLOSS_TILE_BWD_CHUNK 4   /* destination pixels whose derivative a backward workgroup holds in LDS at a time */

typedef struct maskloss_shape {
    int N, h, w, H, W;
} maskloss_shape;

int maskloss_version(void);
const char *maskloss_last_error(void);
int maskloss_tile(int which);       /* -1 for an unknown constant */

/* Bytes of the workspace of maskloss_forward, a multiple of 256; negative on a bad argument: four arithmetic values per
 * (instance, forward tile), or nothing when an instance is one tile.  The backward needs none.  Host arithmetic only. */
long long maskloss_workspace_bytes(int dtype, const maskloss_shape *shape);

/* focal, dice [N] and sums [N, 3], in one or two enqueued passes:
 *   tiles    per (instance, tile of consecutive destination pixels): the source rows the tile's taps touch -> LDS, 16
 *            pixels per lane, the tile's sums of focal, p*t, p and t -> workspace; an instance of one tile writes its
 *            results at once;
 *   combine  per instance: the tiles in a fixed order.
 * workspace: at least maskloss_workspace_bytes() bytes, 16-byte aligned, uninitialised (may be NULL when that is 0).
 * N == 0 is a no-op. */
int maskloss_forward(int dtype, int target_kind, const void *src, const void *target, const maskloss_shape *shape,
                     double alpha, double gamma, void *workspace, void *focal, void *dice, void *sums, void *stream);

/* grad_src [N, h, w], every element written, in one enqueued pass: per (instance, tile of source rows x columns) the
 * derivative g over the destination region the tile's taps cover, a chunk at a time in LDS, gathered per source pixel.
 * N == 0 is a no-op. */
int maskloss_backward(int dtype, int target_kind, const void *src, const void *target, const void *sums,
                      const void *grad_focal, const void *grad_dice, const maskloss_shape *shape, double alpha,
                      double gamma, void *grad_src, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MASKLOSS_H */
