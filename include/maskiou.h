/*
 * maskiou.h -- C ABI of the clip-stitching operators (DeVIS Tracker.process_masks / encode_mask and
 * HungarianInferenceMatcher.compute_volumetric_iou_cost / compute_frame_average_iou_cost) in libmsda_hip.so: the matrix of
 * soft mask IoUs between two sets of small logit maps, and the binarised full-resolution masks, one byte per pixel
 * (DESIGN.md section 12).  Nothing of the target's resolution is ever written to memory in a floating type.
 *
 * Geometry: logit maps of (h, w) pixels, the target size (H, W), F frames, p = h*w, P = H*W, K = F*P.
 *
 * The resampled logit x is exactly the rule of maskloss.h (PyTorch mode="bilinear", align_corners=False, size= given:
 * scale, r, i0, i1, l1, l0 and the four-tap expression stated there), every product and sum rounded on its own, evaluated in
 * float for MASKIOU_F32 / BF16 / F16 and in double for MASKIOU_F64; downsampling and the identity follow the same rule; x is
 * never rounded to a 16-bit type.  One addition for logits that are not finite: a tap whose weight l1 is exactly 0
 * contributes nothing instead of l1 * value.  For finite logits that changes no result (at most the sign of a zero x, which
 * neither sigmoid nor x > 0 sees); it keeps 0 * inf from turning the border pixels of an infinite logit into NaN.
 *
 * p = sigmoid(x) is the expression of maskloss.h: e = exp(-|x|), p = x >= 0 ? 1/(1+e) : e/(1+e).  So +inf gives p = 1,
 * -inf gives p = 0 and a NaN logit gives a NaN p wherever one of its taps has a nonzero weight.
 *
 * maskiou_pairwise: a [Na, F, h, w], b [Nb, F, h, w]; pa[i, f, d] and pb[j, f, d] the probabilities at destination pixel d.
 *   inter[f, i, j] = sum over d of pa[i, f, d] * pb[j, f, d]
 *   sum_a[f, i]    = sum over d of pa[i, f, d]              sum_b[f, j] likewise
 *   MASKIOU_VOLUME:  I = sum_f inter, Sa = sum_f sum_a, Sb = sum_f sum_b (f ascending);  iou = I / max(Sa + Sb - I, eps)
 *   MASKIOU_FRAME:   iou = (sum_f inter_f / max(sum_a_f + sum_b_f - inter_f, eps)) / F      (f ascending)
 * max(u, eps) is u < eps ? eps : u, so a NaN stays a NaN.
 *
 * The order of every sum is fixed by (F, H, W) alone -- there are no float atomics:
 *   - a frame's destination pixels are cut into tiles of MASKIOU_TILE_ROWS x MASKIOU_TILE_COLS pixels, the tiles numbered
 *     row-major, the pixels of a tile row-major; positions of a tile outside the map count as p = 0;
 *   - with T tiles per frame, a split range is t = max(MASKIOU_TILE_SPLIT_TILES, ceil(T / MASKIOU_TILE_MAX_SPLITS))
 *     consecutive tiles, and a frame has S = ceil(T / t) of them;
 *   - inside a split range an entry of inter is one chain acc = fma(pa, pb, acc) from 0 over the range's pixels in that
 *     order (for float arithmetic on the matrix pipe, whose f32-input instruction is bit for bit that chain; for double as
 *     explicit fma), an entry of sum_a or sum_b one chain acc = acc + p;
 *   - the S partials of a frame are added in ascending order, from 0.
 * Hence every result is bitwise reproducible; entry (i, j) has the same bits whatever Na, Nb and its position, alone or
 * inside any larger call; sum_a[f, i] depends on map i alone; inter(a, b) is the transpose of inter(b, a) bit for bit; and
 * a NaN of one map poisons its own row or column only.
 *
 * maskiou_binarize: src [N, h, w] -> out, one byte per pixel: x > 0 ? 1 : 0, x the resampled logit in the arithmetic type.
 * That is sigmoid(x) > 0.5 except for 0 < x below about 6e-8 in float (1.1e-16 in double), where 1/(1+exp(-x)) rounds to
 * 0.5.  NaN gives 0.  MASKIOU_ROW_MAJOR writes [N, H, W]; MASKIOU_COL_MAJOR writes [N, W, H] (each mask in Fortran order,
 * what a run-length encoder of column-major masks reads).  A lane owns 16 consecutive bytes of `out` and writes them as one
 * 16-byte store where they start at a 16-byte aligned address and lie inside one mask, as single bytes otherwise; the
 * bits are the same either way.  `out` needs no alignment.
 *
 * Conventions (those of maskloss.h)
 *   - every pointer is a DEVICE pointer unless stated; tensors are dense; a, b, src in `dtype`, which need element
 *     alignment only; inter [F, Na, Nb], sum_a [F, Na], sum_b [F, Nb], iou [Na, Nb] in the arithmetic type (float; double
 *     for MASKIOU_F64); every element of the four outputs is written;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and
 *     never synchronise (HIP-graph capture works), and are re-entrant;
 *   - element offsets are 64-bit; p, P, F*p, Na*Nb + Na + Nb, and the number of workgroups of a launch must fit 31 bits;
 *   - return value: MASKIOU_OK (0) or a negative maskiou_status; on failure maskiou_last_error() returns a thread-local
 *     message.  Arguments are checked before any HIP call, so argument errors are reported without a GPU.
 */
#ifndef MASKIOU_H
#define MASKIOU_H

#ifdef __cplusplus
extern "C" {
#endif

#define MASKIOU_ABI_VERSION 1

typedef enum maskiou_status { MASKIOU_OK = 0, MASKIOU_ERR_ARGUMENT = -1, MASKIOU_ERR_HIP = -2 } maskiou_status;

typedef enum maskiou_dtype { MASKIOU_F32 = 0, MASKIOU_F64 = 1, MASKIOU_BF16 = 2, MASKIOU_F16 = 3 } maskiou_dtype;

typedef enum maskiou_reduce { MASKIOU_VOLUME = 0, MASKIOU_FRAME = 1 } maskiou_reduce;

typedef enum maskiou_layout { MASKIOU_ROW_MAJOR = 0, MASKIOU_COL_MAJOR = 1 } maskiou_layout;

/* maskiou_tile(): which constant of the kernels' tiling */
#define MASKIOU_TILE_BLOCK 0        /* rows of a and of b per workgroup of the pairwise pass: a BLOCK x BLOCK output block */
#define MASKIOU_TILE_ROWS 1         /* destination rows of a pixel tile */
#define MASKIOU_TILE_COLS 2         /* destination columns of a pixel tile */
#define MASKIOU_TILE_SPLIT_TILES 3  /* the fewest tiles of a split range */
#define MASKIOU_TILE_MAX_SPLITS 4   /* the most split ranges of a frame */
#define MASKIOU_TILE_BIN_PIXELS 5   /* consecutive bytes of `out` per workgroup of maskiou_binarize, 16 per lane */
#define MASKIOU_TILE_BIN_SRC 6      /* source elements a binarise workgroup keeps in LDS; a tile needing more reads memory */

typedef struct maskiou_shape {
    int Na, Nb, F, h, w, H, W;
} maskiou_shape;

int maskiou_version(void);
const char *maskiou_last_error(void);
int maskiou_tile(int which);        /* -1 for an unknown constant */

/* Bytes of the workspace of maskiou_pairwise, a multiple of 256; negative on a bad argument: F * S * (Na*Nb + Na + Nb)
 * arithmetic values (S the split ranges of a frame, above); 0 when Na or Nb is 0.  Host arithmetic only. */
long long maskiou_workspace_bytes(int dtype, const maskiou_shape *shape);

/* inter, sum_a, sum_b and iou in two enqueued passes:
 *   pairwise  per (BLOCK x BLOCK output block, frame, split range): per pixel tile, p of the block's maps -> LDS, once per
 *             (map, pixel); the block's products accumulated from LDS; the range's partials -> workspace;
 *   combine   per entry (i, j): the partials in ascending order, then the ratio.
 * workspace: at least maskiou_workspace_bytes() bytes, 16-byte aligned, uninitialised.  Na == 0 or Nb == 0 is a no-op. */
int maskiou_pairwise(int dtype, int reduce, const void *a, const void *b, const maskiou_shape *shape, double eps,
                     void *workspace, void *inter, void *sum_a, void *sum_b, void *iou, void *stream);

/* out [N, H, W] (MASKIOU_ROW_MAJOR) or [N, W, H] (MASKIOU_COL_MAJOR) bytes, every one written, in one enqueued pass.
 * N == 0 is a no-op. */
int maskiou_binarize(int dtype, int layout, const void *src, int N, int h, int w, int H, int W, void *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MASKIOU_H */
