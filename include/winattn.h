/*
 * winattn.h -- C ABI of the Swin backbone's (shifted-)window attention in libmsda_hip.so: what a
 * SwinTransformerBlock computes between its qkv Linear and its proj Linear -- cyclic shift, window partition, scaled
 * logits, relative-position bias, shift mask, softmax, product with v, window merge and reverse shift -- as index arithmetic
 * around one attention pass, forward and backward.  No window copy, no logit or probability matrix, no mask tensor and no
 * index buffer exists anywhere.
 *
 * Geometry.  qkv [B, Hp, Wp, 3C], dense: the block's qkv Linear applied to the padded, un-rolled, un-partitioned map; channel
 * (part * nH + h) * D + d with part 0 / 1 / 2 = q / k / v (the reference's reshape(..., 3, nH, D)), C = nH * D, D % 4 == 0 and
 * 4 <= D <= WINATTN_MAX_HEAD_DIM.  ws = window, 1 <= ws <= WINATTN_MAX_WINDOW, Hp % ws == 0, Wp % ws == 0, 0 <= shift < ws,
 * N = ws * ws tokens per window, nW = (Hp / ws) * (Wp / ws) windows per map, window w = wy * (Wp / ws) + wx.
 * bias_table [(2 ws - 1)^2, nH], dense.  out [B, Hp, Wp, C], dense, in map order (already rolled back).
 *
 * Addressing.  Token i = iy * ws + ix of window (wy, wx) sits at the shifted coordinates (ys, xs) = (wy * ws + iy, wx * ws + ix)
 * and reads qkv and writes out at map pixel ((ys + shift) mod Hp, (xs + shift) mod Wp).
 *
 * Logits, per batch entry b, window w and head h, for query token i and key token j of that window:
 *     S[i, j] = scale * (q_i . k_j) + table[(iy - jy + ws - 1) * (2 ws - 1) + (ix - jx + ws - 1), h] + mask(i, j)
 *   With shift > 0, mask(i, j) = -100.0 (finite and additive) where region(i) != region(j) and 0 elsewhere, with
 *     region = 3 * r(ys, Hp) + r(xs, Wp)           r(c, n) = (c >= n - ws) + (c >= n - shift)
 *   With shift == 0 there is no mask.
 *     P = softmax over j of S            out_i = sum_j P[i, j] v_j
 *
 * dtypes: one of WINATTN_F32 / BF16 / F16 for qkv, out and grad_qkv; WINATTN_F64 is refused.  bias_table and grad_table have
 * the same dtype, or -- `wide` != 0, the autocast case -- are float32 beside a 16-bit dtype.  Arithmetic is float for every
 * storage dtype (v_mfma_f32_16x16x4_f32 products, the softmax with the row maximum subtracted and rescaled online across key
 * tiles, every sum); a result is rounded once, at the store.  lse [B, nW, nH, N] is float: log of the row sum of exp(S).
 *
 * Backward.  With delta_i = sum_d(dO * O) of row i -- O in float (out_acc) --:
 *     dP = dO V^T        dS = P o (dP - delta)        dQ = scale * dS K        dK = scale * dS^T Q        dV = P^T dO
 *     grad_table[r, h] = sum of dS[b, w, h, i, j] over every b, every w and every (i, j) whose table row is r
 *   grad_qkv given: one pass over query tiles writes part 0 and one over key tiles writes parts 1 and 2; every element of
 *   grad_qkv is written.  grad_table given: a wave owns one head, one query tile and one key tile for a chunk of consecutive
 *   (b, w) windows and keeps the sum of their dS tiles in accumulators (windows ascending); it writes one [chunks, nH, N, N]
 *   float partial into the workspace; a second pass adds the chunks in ascending order into [nH, N, N]; a third folds (i, j) -> r
 *   in ascending (i, j) and rounds once.  The number of chunks is a function of the shape alone (winattn_workspace_bytes).  What
 *   is not asked for is not computed.
 *
 * Kernels (gfx950, wave64): the register map of selfattn.h -- one wave owns 16 rows of one (b, w, h) and walks the other
 * tokens of the window in tiles of 16, the logit tile transposed in the accumulators.  No LDS, no atomics, nothing is zeroed;
 * every loop is counted and every sum has a fixed order that depends on the shape alone, so every result is bitwise
 * reproducible, out and grad_qkv of a batch entry do not depend on the other batch entries, and the 8- to 16-byte path (every
 * pointer 16-byte aligned) and the per-element path give the same bits.
 *
 * Conventions (those of selfattn.h)
 *   - every pointer is a DEVICE pointer; tensors need element alignment only (the workspace: 4 bytes);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and never
 *     synchronise (HIP-graph capture works), and are re-entrant; the caller provides the workspace;
 *   - return value: the number of kernel launches enqueued (>= 0), or a negative winattn_status; on failure
 *     winattn_last_error() returns a thread-local message.  Arguments are checked before any HIP call, so argument errors are
 *     reported without a GPU.
 */
#ifndef WINATTN_H
#define WINATTN_H

#ifdef __cplusplus
extern "C" {
#endif

#define WINATTN_ABI_VERSION 1

typedef enum winattn_status { WINATTN_OK = 0, WINATTN_ERR_ARGUMENT = -1, WINATTN_ERR_HIP = -2 } winattn_status;

typedef enum winattn_dtype { WINATTN_F32 = 0, WINATTN_F64 = 1, WINATTN_BF16 = 2, WINATTN_F16 = 3 } winattn_dtype;

#define WINATTN_MAX_HEAD_DIM 64
#define WINATTN_MAX_WINDOW 16

typedef struct winattn_shape {
    long long B;            /* batch entries */
    long long Hp;           /* rows of the padded map: a multiple of window */
    long long Wp;           /* columns of the padded map: a multiple of window */
    long long heads;        /* nH */
    long long head_dim;     /* D */
    long long window;       /* ws */
    long long shift;        /* 0 <= shift < ws */
} winattn_shape;

int winattn_version(void);
const char *winattn_last_error(void);

/* Bytes of the workspace winattn_backward needs when grad_table is given: (chunks + 1) * nH * N * N floats.  Host arithmetic
 * only.  A negative winattn_status for a bad shape. */
long long winattn_workspace_bytes(const winattn_shape *shape);

/* out [B, Hp, Wp, C], every element written, in one enqueued pass; when given (a backward will follow), lse [B, nW, nH, N]
 * float and out_acc [B, Hp, Wp, C] FLOAT: out before its rounding to a 16-bit dtype (with WINATTN_F32 out is that already and
 * out_acc may stay NULL).  Returns 1, or 0 for an empty problem (B, Hp or Wp is 0), which dereferences nothing. */
int winattn_forward(int dtype, int wide, const void *qkv, const void *bias_table, double scale, const winattn_shape *shape,
                    void *out, void *lse, void *out_acc, void *stream);

/* The gradients that are given: grad_qkv [B, Hp, Wp, 3C] in the storage dtype and grad_table [(2 ws - 1)^2, nH] in the table's,
 * every element written.  out_acc [B, Hp, Wp, C] is FLOAT for every dtype -- the forward's out_acc, or its out with
 * WINATTN_F32 --, grad_out is dense [B, Hp, Wp, C] in the storage dtype, lse is the forward's.  `workspace` is required with
 * grad_table.  Returns the number of passes enqueued: 2 for grad_qkv plus 3 for grad_table, 0 when no gradient is asked for or
 * the problem is empty (the caller provides the zeros). */
int winattn_backward(int dtype, int wide, const void *qkv, const void *bias_table, const void *out_acc, const void *grad_out,
                     const void *lse, double scale, const winattn_shape *shape, void *grad_qkv, void *grad_table,
                     void *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* WINATTN_H */
