/*
 * selfattn.h -- C ABI of the decoder's query self-attention in libmsda_hip.so: what
 * nn.MultiheadAttention computes between its input projections and out_proj,
 *
 *     for every batch entry n and head h over the channels h*D .. h*D+D-1, D = E / H:
 *         S   = (q_h k_h^T) / sqrt(D)                  [L, S]
 *         P   = softmax over the keys of S
 *         out = dropout_p(P) v_h                       [L, D]
 *
 * forward and backward.  No probability matrix and no mask is ever stored: the forward keeps one float per row (lse) and,
 * for 16-bit dtypes, out before its rounding (out_acc); the backward recomputes P from lse and the mask from the seed.
 *
 * Geometry: q [L, N, E], k and v [S, N, E], out [L, N, E]; H heads of D = E / H channels with D % 4 == 0 and
 * 4 <= D <= SELFATTN_MAX_HEAD_DIM.  q, k and v are VIEWS: each has a sequence stride and a batch stride in ELEMENTS
 * (selfattn_view) and a channel stride that must be 1 -- so q and k may be the two column halves of one [L, N, 2E] GEMM
 * result, and a batch_first tensor is the view with the two strides exchanged.  out, lse and every gradient are dense.
 * L, S, N, E and every stride must fit 31 bits; element offsets are 64-bit.
 *
 * dtypes: one of SELFATTN_F32 / BF16 / F16 for q, k, v, out and the gradients; SELFATTN_F64 is refused.  Arithmetic is float
 * for every storage dtype -- 16-bit operands are converted at the load --: the products (v_mfma_f32_16x16x4_f32: an exact
 * float fma chain), the softmax with the row maximum subtracted and rescaled online across key tiles, and every sum.  A
 * result is rounded once, at the store.  lse [N * H, L] is float: row maximum plus log of the row sum of the scaled logits.
 *
 * The mask.  p is the probability of dropping a probability (after the softmax, as torch does).  On the host, in double:
 *     threshold = floor(p * 2^32), a 64-bit integer in [0, 2^32]        scale = 1 / (1 - p), and 0 for p == 1
 *   `seed` is a DEVICE pointer to one int64 the kernels read; it is never read on the host, so a captured HIP graph replayed
 *   after the seed was overwritten draws a new mask.  With p == 0 there is no mask, `seed` is ignored and may be NULL.
 *   Probability (n, h, i, j) -- query i, key j -- is KEPT iff word >= threshold, where word is output word (j & 3) of
 *     Philox4x32-10( key     = (seed & 0xffffffff, seed >> 32),
 *                    counter = (row & 0xffffffff, row >> 32, j >> 2, 1) ),      row = (n * H + h) * L + i
 *   The generator and the threshold are those of addnorm.h; the last counter word is 1 where addnorm.h has 0, so the two
 *   streams are disjoint under an equal seed.  p == 1 keeps nothing (no word reaches 2^32) and out is exactly 0.
 *
 * Backward.  With delta_i = sum_d(dO * O) of row i -- O in float, out_acc: delta cancels against dP, and an O rounded to
 * bfloat16 costs percents of grad_q and grad_k once the softmax is peaked -- and keep / scale as above:
 *     dP = keep * scale * (dO V^T)          dS = P o (dP - delta)            (the identity holds with dropout as well)
 *     dQ = dS K / sqrt(D)                   dK = dS^T Q / sqrt(D)            dV = dropout(P)^T dO
 *   At most two enqueued passes: one over query tiles that loops over the keys and writes grad_q, one over key tiles that
 *   loops over the queries and writes grad_k and / or grad_v.  Each output pointer may be NULL: what is not asked for is not
 *   computed (grad_q alone: one pass; grad_k and / or grad_v: the other; none: nothing is enqueued and 0 is returned).
 *
 * Kernels (gfx950, wave64).  One wave owns 16 rows of one (n, h) and walks the other sequence in tiles of 16.  The logit tile is
 * computed TRANSPOSED, S^T [16 keys x 16 queries] = K Q^T, so that in the accumulator map (col = lane & 15, row = 4 * (lane >>
 * 4) + reg) a query is a lane column: its row statistics are a reduction over 4 registers and the lanes i, i+16, i+32, i+48,
 * and the tile in registers is already the B operand of O^T [16 channels x 16 queries] += V^T P^T, with k-slot lane >> 4 of
 * step r being key 4 * (lane >> 4) + r.  The backward chains the same way (dP^T = V dO^T, dQ^T += K^T dS^T; the key-tile pass
 * uses the untransposed tile for dV^T += dO^T P and dK^T += Q^T dS).  No LDS, no atomics, nothing is zeroed; every loop is
 * counted and every sum has a fixed order that depends on the shape alone, so every result is bitwise reproducible, does not
 * depend on the other batch entries or heads, and is the same for the 8- to 16-byte path (every pointer 16-byte aligned and
 * every stride a multiple of 4 elements) and the per-element path.  NaN and inf propagate as in torch: a NaN query row
 * poisons that row, a NaN key its (n, h).
 *
 * Conventions (those of addnorm.h)
 *   - every pointer is a DEVICE pointer; tensors need element alignment only;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and never
 *     synchronise (HIP-graph capture works), and are re-entrant; no workspace is needed;
 *   - return value: the number of kernel launches enqueued (>= 0), or a negative selfattn_status; on failure
 *     selfattn_last_error() returns a thread-local message.  Arguments are checked before any HIP call, so argument errors are
 *     reported without a GPU.
 */
#ifndef SELFATTN_H
#define SELFATTN_H

#ifdef __cplusplus
extern "C" {
#endif

#define SELFATTN_ABI_VERSION 2

typedef enum selfattn_status { SELFATTN_OK = 0, SELFATTN_ERR_ARGUMENT = -1, SELFATTN_ERR_HIP = -2 } selfattn_status;

typedef enum selfattn_dtype { SELFATTN_F32 = 0, SELFATTN_F64 = 1, SELFATTN_BF16 = 2, SELFATTN_F16 = 3 } selfattn_dtype;

#define SELFATTN_MAX_HEAD_DIM 64

typedef struct selfattn_shape {
    long long L;            /* queries */
    long long S;            /* keys */
    long long N;            /* batch entries */
    long long E;            /* channels: H * D */
    long long H;            /* heads */
} selfattn_shape;

typedef struct selfattn_view {
    long long seq;          /* elements between consecutive positions of the sequence */
    long long batch;        /* elements between consecutive batch entries */
    long long channel;      /* elements between consecutive channels: must be 1 */
} selfattn_view;

int selfattn_version(void);
const char *selfattn_last_error(void);

/* out [L, N, E], every element written, in one enqueued pass; when given (a backward will follow), lse [N * H, L] float and
 * out_acc [L, N, E] FLOAT, dense: out before its rounding to a 16-bit dtype (with SELFATTN_F32 out is that already and
 * out_acc may stay NULL).  Returns 1.  L == 0 or N == 0: nothing to write, returns 0.  S == 0: returns 0 and writes nothing
 * -- the result is zeros, which the caller provides.  Neither dereferences anything. */
int selfattn_forward(int dtype, const void *q, const selfattn_view *q_view, const void *k, const selfattn_view *k_view,
                     const void *v, const selfattn_view *v_view, const long long *seed, double p, const selfattn_shape *shape,
                     void *out, void *lse, void *out_acc, void *stream);

/* The gradients that are given -- grad_q [L, N, E], grad_k and grad_v [S, N, E], dense --, every element written.  out_acc
 * [L, N, E] is FLOAT for every dtype -- the forward's out_acc, or its out with SELFATTN_F32 --, grad_out is dense [L, N, E] in
 * the storage dtype, lse is the forward's.  Returns the number of passes enqueued: 0 when no gradient is asked for or the
 * problem is empty (L, S or N is 0: the caller provides the zeros), else 1 or 2. */
int selfattn_backward(int dtype, const void *q, const selfattn_view *q_view, const void *k, const selfattn_view *k_view,
                      const void *v, const selfattn_view *v_view, const void *out_acc, const void *grad_out, const void *lse,
                      const long long *seed, double p, const selfattn_shape *shape, void *grad_q, void *grad_k, void *grad_v,
                      void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SELFATTN_H */
