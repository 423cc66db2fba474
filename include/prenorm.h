/*
 * prenorm.h -- C ABI of the glue of the Swin backbone's blocks in libmsda_hip.so: what the reference's
 * SwinTransformerBlock, BasicLayer and PatchMerging (src/models/swin_backbone.py) compute around their Linears and the window
 * attention -- the residual add with its drop-path scale, the pre-norm LayerNorm, the copy into the zero-padded window map and
 * the 2 x 2 patch gather -- as one pass forward (prenorm_forward) and one backward (prenorm_backward).
 *
 * The row.  A call normalises R rows z[r, :] of C channels, 1 <= C <= PRENORM_MAX_CHANNELS (a row lives in the registers of one
 * wave).  The batch has B entries; an entry has H * W source tokens, row-major.  prenorm_shape.source says where a row comes
 * from:
 *   PRENORM_PLAIN     R = B * H * W.  z = A(x[r]).
 *   PRENORM_RESIDUAL  R = B * H * W.  k = keep[b(r)], b(r) = r / (H * W), from the optional float32 vector keep [B] (the
 *                     drop-path scale: 0 or 1 / keep_prob); k = 1 when keep is NULL.
 *                       t = k != 0 ? A(x[r]) + A(delta[r]) * k : A(x[r])      (a row with k == 0 takes exactly x, whatever delta
 *                                                                              holds -- addnorm.h's rule for a dropped element,
 *                                                                              not x + delta * 0; delta is not read there)
 *                       s[r] = t rounded to x's dtype, written as a second output [R, C]: the residual stream
 *                       z = A(s[r])                                           (for float32 x, z = t)
 *   PRENORM_MERGE     x is [B, H, W, C / 4]; R = B * H2 * W2 with H2 = ceil(H / 2), W2 = ceil(W / 2).  Row (b, i, j) is the
 *                     concatenation of x[b, 2i, 2j], x[b, 2i+1, 2j], x[b, 2i, 2j+1], x[b, 2i+1, 2j+1] -- the order of
 *                     PatchMerging.forward --, C / 4 channels each, a piece being 0 where its position lies outside H x W.
 *                     C must be a multiple of 4.  No padded or concatenated tensor exists.
 *
 * The norm.  A is float for every storage dtype.  Every product and sum is rounded on its own (no fused multiply-add); eps is
 * rounded to A once.
 *     mean = sum_c(z) / C
 *     var  = sum_c((z - mean)^2) / C                 (a second pass over the registers)
 *     rstd = 1 / sqrt(var + eps)
 *     y    = ((z - mean) * rstd) * weight + bias     rounded once, at the store
 *   Order of the sums over C (addnorm.h's): lane l of the wave owns the channels (g * 64 + l) * 4 + j for g = 0.. and j = 0..3
 *   and adds them with g, then j, ascending (channels >= C count as 0); the 64 lanes are combined by butterflies (xor 32, 16,
 *   .. 1), so every lane has the same bits.  The order depends on C alone -- not on the load width, the alignment, the source
 *   or destination form or the launch geometry: the 16-byte path and the per-element path give the same bits.
 *   mean and rstd [R], float32, are written when the pointers are given (a backward will follow).
 *
 * The destination of y.  prenorm_shape.dest:
 *   PRENORM_TOKENS    y is [R, C], dense.
 *   PRENORM_MAP       y is [B, Hp, Wp, C] with Hp >= H and Wp >= W (not with PRENORM_MERGE): the row of token (b, h, w) goes to
 *                     map position (b, h, w), and every element of every other position is written as exactly 0 by the same
 *                     launch -- norm1 and F.pad in one pass.
 *
 * Backward.  grad_y has y's layout (the padding positions of a map are not read); grad_s [R, C], x's dtype, is optional (NULL:
 * zero, and always NULL outside PRENORM_RESIDUAL).  `x` is what z is read from: x itself in PLAIN and MERGE (re-gathered), the
 * forward's s in RESIDUAL -- delta is not an input.  With xhat = (z - mean) * rstd from the saved mean and rstd, g = A(grad_y),
 * gw = g * weight:
 *     c1 = sum_c(gw) / C        c2 = sum_c(gw * xhat) / C             (the forward's order)
 *     dz = ((gw - c1) - xhat * c2) * rstd + A(grad_s)
 *     grad_x = dz               grad_delta = k != 0 ? dz * k : 0      (keep is data, not a differentiable operand)
 *     grad_weight[c] = sum_r(g * xhat)       grad_bias[c] = sum_r(g)
 *   In MERGE grad_x is [B, H, W, C / 4]: every input element belongs to exactly one row, so each is written once, without
 *   atomics; the gradient of a padded piece is dropped.
 *   The two column sums have a fixed order: rows are cut into chunks of prenorm_tile(PRENORM_TILE_ROWS) consecutive rows; a wave
 *   adds its chunk's rows ascending in registers and writes one partial per column to the workspace; a combine launch has one
 *   wave per column, whose lane l adds the chunks l, l + 64, l + 128, .. ascending, the 64 lanes are combined by the
 *   butterflies above, and the sum is rounded once to the parameters' dtype.  A call of one chunk writes the results itself: one
 *   launch.  Each output pointer may be NULL: what is not asked for is not computed (grad_weight and grad_bias both NULL: no
 *   partials, no combine, no workspace).
 *
 * dtypes.  prenorm_types names the dtype of x (and s, grad_x, grad_s), of delta (and grad_delta), of y (and grad_y) and of
 * weight / bias (and their gradients), among F32, BF16 and F16:
 *   - one dtype for all four;
 *   - beside F32 x, s and parameters: a 16-bit delta, a 16-bit y, or both in one 16-bit dtype (autocast: a 16-bit GEMM result
 *     added to a float32 stream, and a y the next autocast Linear reads without a cast pass);
 *   - F32 parameters beside 16-bit everything else.
 *   Everything else is refused; float64 is not a kernel dtype.  In PLAIN and MERGE there is no delta and types.delta must equal
 *   types.x.
 *
 * Kernels (gfx950, wave64): one wave owns a row and holds it in registers; loads and stores are 8 to 16 bytes per lane when
 * C % 4 == 0 (MERGE: (C / 4) % 4 == 0) and every operand is 16-byte aligned, per element otherwise.  No LDS, no atomics,
 * nothing is zeroed by a pass of its own: every output element is written by the launch that owns it.
 *
 * Conventions (those of addnorm.h)
 *   - every pointer is a DEVICE pointer; tensors are dense and need element alignment only;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and never
 *     synchronise (HIP-graph capture works), and are re-entrant;
 *   - element offsets are 64-bit; R and B * Hp * Wp must fit 31 bits;
 *   - return value: PRENORM_OK (0) or a negative prenorm_status; on failure prenorm_last_error() returns a thread-local
 *     message.  Arguments are checked before any HIP call, so argument errors are reported without a GPU.
 */
#ifndef PRENORM_H
#define PRENORM_H

#ifdef __cplusplus
extern "C" {
#endif

#define PRENORM_ABI_VERSION 1

typedef enum prenorm_status { PRENORM_OK = 0, PRENORM_ERR_ARGUMENT = -1, PRENORM_ERR_HIP = -2 } prenorm_status;

/* (code 1, float64 elsewhere in this library, is refused) */
typedef enum prenorm_dtype { PRENORM_F32 = 0, PRENORM_BF16 = 2, PRENORM_F16 = 3 } prenorm_dtype;

typedef enum prenorm_source { PRENORM_PLAIN = 0, PRENORM_RESIDUAL = 1, PRENORM_MERGE = 2 } prenorm_source;

typedef enum prenorm_dest { PRENORM_TOKENS = 0, PRENORM_MAP = 1 } prenorm_dest;

#define PRENORM_MAX_CHANNELS 3072       /* Swin-L's largest merge row, 4 * 768 */

/* prenorm_tile(): which constant of the kernels' tiling */
#define PRENORM_TILE_ROWS 0         /* rows of one chunk of the backward's column sums */
#define PRENORM_TILE_CHANNELS 1     /* PRENORM_MAX_CHANNELS */

typedef struct prenorm_shape {
    long long B;            /* batch entries */
    int H, W;               /* source tokens of an entry: H rows of W (a caller without a map passes H = 1) */
    int C;                  /* channels of a ROW (in MERGE four times x's channels) */
    int Hp, Wp;             /* PRENORM_MAP: the map's size; ignored otherwise */
    int source, dest;       /* prenorm_source, prenorm_dest */
} prenorm_shape;

typedef struct prenorm_types {
    int x, delta, y, param; /* prenorm_dtype codes */
} prenorm_types;

int prenorm_version(void);
const char *prenorm_last_error(void);
int prenorm_tile(int which);        /* -1 for an unknown constant */

/* Rows R of a shape; negative on a bad argument.  Host arithmetic only. */
long long prenorm_rows(const prenorm_shape *shape);

/* Bytes of the workspace of prenorm_backward when grad_weight or grad_bias is asked for, a multiple of 256; negative on a bad
 * argument: chunks * 2 * C floats, or 0 when the call is one chunk.  Host arithmetic only. */
long long prenorm_workspace_bytes(const prenorm_shape *shape);

/* y, every element written (a map's padding included), and in RESIDUAL s [R, C], in one enqueued pass; mean and rstd [R] when
 * given (both or neither).  delta and s are required in RESIDUAL and must be NULL otherwise; keep may be given in RESIDUAL only.
 * A call without rows and without map positions is a no-op that dereferences and writes nothing. */
int prenorm_forward(const prenorm_types *types, const void *x, const void *delta, const float *keep, const void *weight,
                    const void *bias, double eps, const prenorm_shape *shape, void *s, void *y, float *mean, float *rstd,
                    void *stream);

/* The gradients that are given, every element written, in one enqueued pass, two when the column sums span chunks.
 * workspace: at least prenorm_workspace_bytes() bytes, 16-byte aligned, uninitialised (may be NULL when that is 0 or when
 * neither grad_weight nor grad_bias is given).  grad_delta, grad_s and keep may be given in RESIDUAL only.  All four outputs
 * NULL is an argument error.  R == 0 is a no-op. */
int prenorm_backward(const prenorm_types *types, const void *x, const float *keep, const void *weight, const float *mean,
                     const float *rstd, const void *grad_y, const void *grad_s, const prenorm_shape *shape, void *workspace,
                     void *grad_x, void *grad_delta, void *grad_weight, void *grad_bias, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PRENORM_H */
