/*
 * addnorm.h -- C ABI of the glue between the transformer layers' GEMMs in libmsda_hip.so: what the
 * reference's DeformableTransformerEncoderLayer / DecoderLayer compute between their attention modules and Linears,
 *
 *     y = LayerNorm(x + dropout_p(delta))            (addnorm_forward / addnorm_backward)
 *     y = dropout_p(relu(x))                         (addnorm_relu_forward / addnorm_relu_backward)
 *
 * each as one pass.  No byte mask, no pre-norm sum and no second copy of anything is kept: the backward recomputes both from
 * the operands and the seed.
 *
 * Geometry: R rows of C channels, dense, the caller's leading dimensions flattened.  The norm needs 1 <= C <=
 * ADDNORM_MAX_CHANNELS (a row lives in the registers of one wave); the relu pass takes any C >= 1.
 *
 * The mask (both operators).  p is the probability of dropping.  On the host, in double:
 *     threshold = floor(p * 2^32), a 64-bit integer in [0, 2^32]        scale = 1 / (1 - p), and 0 for p == 1
 *   `seed` is a DEVICE pointer to one int64 the kernels read; it is never read on the host, so a captured HIP graph replayed
 *   after the seed was overwritten draws a new mask.  With p == 0 there is no mask, `seed` is ignored and may be NULL.
 *   Element (row, c) is KEPT iff word >= threshold, where word is output word (c & 3) of
 *     Philox4x32-10( key     = (seed & 0xffffffff, seed >> 32),
 *                    counter = (row & 0xffffffff, row >> 32, c >> 2, 0) )
 *   -- one call serves the four consecutive channels a lane loads.  p == 1 keeps nothing (no word reaches 2^32).
 *   Philox4x32-10 is the generator of Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC'11): multipliers
 *   0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds.
 *
 * The norm.  A is the arithmetic type: float, double for ADDNORM_F64.  Every product and sum is rounded on its own (no fused
 * multiply-add); scale and eps are rounded to A once.
 *     d    = keep ? A(delta) * scale : 0             (a dropped element is exactly 0, whatever delta holds)
 *     z    = A(x) + d
 *     mean = sum_c(z) / C
 *     var  = sum_c((z - mean)^2) / C                 (a second pass over the registers)
 *     rstd = 1 / sqrt(var + eps)
 *     y    = ((z - mean) * rstd) * weight + bias     rounded once, at the store
 *   Order of the sums over C: lane l of the wave owns the channels (g * 64 + l) * 4 + j for g = 0.. and j = 0..3 and adds them
 *   with g, then j, ascending (channels >= C count as 0); the 64 lanes are combined by butterflies (xor 32, 16, .. 1), so
 *   every lane has the same bits.  The order depends on C alone -- not on the load width, the alignment or the launch
 *   geometry: the 16-byte path and the per-element path give the same bits.
 *   mean and rstd [R], in A, are written when the pointers are given (a backward will follow).
 *
 *   Backward, with z recomputed by the forward's operations (the same bits), xhat = (z - mean) * rstd from the saved mean and
 *   rstd, g = A(grad_y), gw = g * weight:
 *     c1 = sum_c(gw) / C        c2 = sum_c(gw * xhat) / C             (the forward's order)
 *     dz = ((gw - c1) - xhat * c2) * rstd
 *     grad_x = dz                grad_delta = keep ? dz * scale : 0
 *     grad_weight[c] = sum_r(g * xhat)       grad_bias[c] = sum_r(g)
 *   The two column sums have a fixed order: rows are cut into chunks of addnorm_tile(ADDNORM_TILE_ROWS) consecutive rows; a
 *   wave adds its chunk's rows ascending in registers and writes one partial per column to the workspace; a combine launch
 *   adds the chunks ascending and rounds once to the parameters' dtype.  A call of one chunk writes the results itself: one
 *   launch.  Each output pointer may be NULL: what is not asked for is not computed (grad_weight and grad_bias both NULL: no
 *   partials, no combine, no workspace).
 *
 * The relu pass.  y = keep ? (x > 0 ? A(x) * scale : (x != x ? x : 0)) : 0 in x's dtype: a dropped element is exactly 0, a
 * kept NaN stays NaN.  The mask rule above holds with row = flat index / C.
 *   Backward: grad_x = y > 0 ? A(grad_y) * scale : 0, from y alone.  This is exact because a kept x > 0 implies y > 0 in
 *   every dtype: scale >= 1, so the product A(x) * scale, rounded to A, is >= A(x) (rounding is monotonic and A(x) itself is
 *   representable); A(x) is a value of the storage type T, so rounding the product to T -- monotonic again -- gives a value
 *   >= x > 0, or +inf on overflow, which is > 0 too.  And y > 0 implies a kept x > 0, since every other case stores 0 or NaN.
 *
 * dtypes.  addnorm_types names the dtype of x, of delta, of y (and grad_y) and of weight / bias (and their gradients):
 *   - one dtype for all four, any of F32 / F64 / BF16 / F16;
 *   - a 16-bit delta beside F32 x, y and parameters (autocast: a 16-bit GEMM result added to a float32 stream);
 *   - 16-bit x and delta with F32 y;
 *   - beside 16-bit x the parameters may be F32.
 *   Everything else is refused.  The relu pass has one dtype.
 *
 * Kernels (gfx950, wave64): one wave owns a row and holds it in registers; loads and stores are 8 to 16 bytes per lane when
 * C % 4 == 0 and every operand is 16-byte aligned, per element otherwise.  No LDS, no atomics, nothing is zeroed.
 *
 * Conventions (those of labelloss.h / posembed.h)
 *   - every pointer is a DEVICE pointer; tensors are dense and need element alignment only;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and never
 *     synchronise (HIP-graph capture works), and are re-entrant;
 *   - element offsets are 64-bit; R must fit 31 bits;
 *   - return value: ADDNORM_OK (0) or a negative addnorm_status; on failure addnorm_last_error() returns a thread-local
 *     message.  Arguments are checked before any HIP call, so argument errors are reported without a GPU.
 */
#ifndef ADDNORM_H
#define ADDNORM_H

#ifdef __cplusplus
extern "C" {
#endif

#define ADDNORM_ABI_VERSION 1

typedef enum addnorm_status { ADDNORM_OK = 0, ADDNORM_ERR_ARGUMENT = -1, ADDNORM_ERR_HIP = -2 } addnorm_status;

typedef enum addnorm_dtype { ADDNORM_F32 = 0, ADDNORM_F64 = 1, ADDNORM_BF16 = 2, ADDNORM_F16 = 3 } addnorm_dtype;

#define ADDNORM_MAX_CHANNELS 1024

/* addnorm_tile(): which constant of the kernels' tiling */
#define ADDNORM_TILE_ROWS 0         /* rows of one chunk of the backward's column sums */
#define ADDNORM_TILE_CHANNELS 1     /* ADDNORM_MAX_CHANNELS */

typedef struct addnorm_shape {
    long long R;            /* rows */
    int C;                  /* channels */
} addnorm_shape;

typedef struct addnorm_types {
    int x, delta, y, param; /* addnorm_dtype codes */
} addnorm_types;

int addnorm_version(void);
const char *addnorm_last_error(void);
int addnorm_tile(int which);        /* -1 for an unknown constant */

/* Bytes of the workspace of addnorm_backward when grad_weight or grad_bias is asked for, a multiple of 256; negative on a
 * bad argument: chunks * 2 * C values of A, or 0 when the call is one chunk.  Host arithmetic only. */
long long addnorm_workspace_bytes(int x_dtype, const addnorm_shape *shape);

/* y [R, C], every element written, in one enqueued pass; mean and rstd [R] in A when given (both or neither).
 * R == 0 is a no-op that dereferences and writes nothing. */
int addnorm_forward(const addnorm_types *types, const void *x, const void *delta, const void *weight, const void *bias,
                    const long long *seed, double p, double eps, const addnorm_shape *shape, void *y, void *mean, void *rstd,
                    void *stream);

/* The gradients that are given, every element written, in one enqueued pass, two when the column sums span chunks.
 * workspace: at least addnorm_workspace_bytes() bytes, 16-byte aligned, uninitialised (may be NULL when that is 0 or when
 * neither grad_weight nor grad_bias is given).  All four outputs NULL is an argument error.  R == 0 is a no-op. */
int addnorm_backward(const addnorm_types *types, const void *x, const void *delta, const void *weight, const long long *seed,
                     double p, const void *mean, const void *rstd, const void *grad_y, const addnorm_shape *shape,
                     void *workspace, void *grad_x, void *grad_delta, void *grad_weight, void *grad_bias, void *stream);

/* y [R, C] in `dtype`, every element written, in one enqueued pass.  R == 0 is a no-op. */
int addnorm_relu_forward(int dtype, const void *x, const long long *seed, double p, const addnorm_shape *shape, void *y,
                         void *stream);

/* grad_x [n] from y and grad_y [n] (n = R * C, flat), every element written, in one enqueued pass.  n == 0 is a no-op. */
int addnorm_relu_backward(int dtype, const void *y, const void *grad_y, double p, long long n, void *grad_x, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ADDNORM_H */
