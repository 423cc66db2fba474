/*
 * inputproj.h -- C ABI of the encoder's input projections in libmsda_hip.so: the GroupNorm of the
 * reference's input_proj[l] = Sequential(Conv2d, GroupNorm(32, hidden_dim)) (src/models/deformable_detr.py) of every pyramid
 * level, written once, channels last, at the level's token offset -- what DeformableTransformer.prepare_data
 * (src/models/deformable_transformer.py) builds as src_flatten = cat([GroupNorm_l(x_l).flatten(2).transpose(1, 2)], 1).  The
 * convolutions stay where they are; no normalised NCHW map exists, forward or backward.
 *
 * ---- inputproj: x_l [N, C, H_l, W_l], l = 0 .. L - 1  ->  tokens [N, S, C], S = sum_l H_l * W_l -----------------------------
 * 1 <= L <= INPUTPROJ_MAX_LEVELS, 1 <= C <= INPUTPROJ_MAX_CHANNELS, C % G == 0; cpg = C / G.  HW_l = H_l * W_l,
 * start_l = sum_{k < l} HW_k, M_l = cpg * HW_l (the elements of a group, one contiguous run of x_l).  A is float for every
 * storage dtype.
 *   Statistics of group (n, l, g), the elements e = 0 .. M_l - 1 of the run that starts at x_l[n, g * cpg, 0, 0]:
 *       The run is cut into chunks of inputproj_tile(INPUTPROJ_TILE_STAT_CHUNK) elements, the last one partial.  Of a chunk with
 *       cnt elements: m = sum(A(x)) / cnt, M2 = sum((A(x) - m)^2) -- two sweeps over the registers, never E[x^2] - E[x]^2.  Order
 *       of both sums: a thread (of 256) adds its elements ascending -- thread t owns the elements i * 256 * V + t * V + j,
 *       j = 0 .. V - 1, i ascending, V = 16 / sizeof(x's dtype) --, then butterflies over the lanes (xor 32 .. 1), then the four
 *       waves ascending.  The chunks k = 0, 1, .. are combined ascending (Chan): with (nA, mA, M2A) the combination so far and
 *       (nB, mB, M2B) the next chunk, d = mB - mA, n = nA + nB: mA += d * (nB / n), M2A += M2B + (d * d) * (nA * (nB / n)).
 *       mean = mA, rstd = 1 / sqrt(M2A / M_l + eps).  mean and rstd are [N, L, G], float32.  A group of one chunk is written by
 *       the statistics launch itself; others by a combine launch.
 *   tokens[n, start_l + p, c] = ((A(x_l[n, c, p]) - mean) * rstd) * A(weight_l[c]) + A(bias_l[c]), rounded once at the store,
 *       with mean and rstd of group c / cpg.  The bits of a token do not depend on N, on the other levels, on the alignment of
 *       the operands or on the launch geometry.
 *   Backward.  g = A(grad_tokens[n, start_l + p, c]), xhat = (A(x) - mean) * rstd from the saved statistics:
 *           A_[n, c] = sum_p(g), B_[n, c] = sum_p(g * xhat)
 *           grad_bias_l[c] = sum_n(A_), grad_weight_l[c] = sum_n(B_)                 (n ascending, rounded once)
 *           c1[n, g] = sum_{c in g}(A(weight_l[c]) * A_[n, c]) / M_l, c2[n, g] = sum_{c in g}(A(weight_l[c]) * B_[n, c]) / M_l
 *                                                                                       (c ascending)
 *           grad_x_l[n, c, p] = ((g * A(weight_l[c]) - c1) - xhat * c2) * rstd        (dense NCHW, x_l's dtype, rounded once)
 *       Order of the sums over the pixels: the pixels of a level are cut into chunks of inputproj_tile(INPUTPROJ_TILE_SUM_CHUNK),
 *       a chunk into tiles of inputproj_tile(INPUTPROJ_TILE_PIXELS).  Lane p of the wave that owns channel c adds the pixels
 *       tile * 64 + p of its chunk, tiles ascending; butterflies (xor 32 .. 1) give the chunk's partial; a combine launch adds
 *       the chunks ascending.  Three enqueued passes (sums, combine, grad_x); without any grad_x two.  No atomics, nothing is
 *       zeroed: every output element is written by the launch that owns it.  Each of the 3 L output pointers may be NULL: what
 *       is not asked for is not computed (a level with no output takes part in no pass).
 *   dtypes (inputproj_types: x and grad_x; param = every weight, bias and their gradients; y = tokens and grad_tokens):
 *       x F32: param F32, y any of the three.  x BF16 / F16: param x's dtype or F32, y x's dtype or F32.
 *
 * Kernels (gfx950, wave64, 256 threads).  apply / sums / grad_x: a workgroup owns a tile of 64 pixels x 64 channels of one
 * frame of one level, held in LDS as [64 channels][64 pixels], row pitch 65 floats.  The map side is read and written along
 * the pixels (256-byte runs per channel, float32); the token side along the channels, V = 16 / sizeof(y's dtype) channels per
 * thread in one 16-byte access where C % V == 0 and the tensor is 16-byte aligned, else per element (the same bits).  On the
 * token side the 32 lanes of half a wave hold 32 / V channel quads x V pixels, so that their LDS accesses fall into 32
 * different banks.
 *
 * Conventions (those of swinends.h)
 *   - every pointer is a DEVICE pointer (the inputproj_levels tables themselves are host structs of device pointers); tensors
 *     are dense and need element alignment only;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and never
 *     synchronise (HIP-graph capture works), and are re-entrant;
 *   - element offsets are 64-bit; M_l and N * S must fit 31 bits;
 *   - return value: INPUTPROJ_OK (0) or a negative inputproj_status; on failure inputproj_last_error() returns a thread-local
 *     message.  Arguments are checked before any HIP call, so argument errors are reported without a GPU.
 */
#ifndef INPUTPROJ_H
#define INPUTPROJ_H

#ifdef __cplusplus
extern "C" {
#endif

#define INPUTPROJ_ABI_VERSION 1

typedef enum inputproj_status { INPUTPROJ_OK = 0, INPUTPROJ_ERR_ARGUMENT = -1, INPUTPROJ_ERR_HIP = -2 } inputproj_status;

/* (code 1, float64 elsewhere in this library, is refused) */
typedef enum inputproj_dtype { INPUTPROJ_F32 = 0, INPUTPROJ_BF16 = 2, INPUTPROJ_F16 = 3 } inputproj_dtype;

#define INPUTPROJ_MAX_LEVELS 8
#define INPUTPROJ_MAX_CHANNELS 1024

/* inputproj_tile(): which constant of the kernels' tiling */
#define INPUTPROJ_TILE_PIXELS 0         /* pixels of a workgroup's tile */
#define INPUTPROJ_TILE_CHANNELS 1       /* channels of a workgroup's tile */
#define INPUTPROJ_TILE_STAT_CHUNK 2     /* elements of a chunk of a group's statistics */
#define INPUTPROJ_TILE_SUM_CHUNK 3      /* pixels of a chunk of the backward's per-channel sums */
#define INPUTPROJ_TILE_MAX_LEVELS 4     /* INPUTPROJ_MAX_LEVELS */
#define INPUTPROJ_TILE_MAX_CHANNELS 5   /* INPUTPROJ_MAX_CHANNELS */

typedef struct inputproj_shape {
    long long N;                        /* frames */
    int C, G, L;                        /* channels, groups, levels */
    int H[INPUTPROJ_MAX_LEVELS], W[INPUTPROJ_MAX_LEVELS];
} inputproj_shape;

typedef struct inputproj_types {
    int x, param, y;                    /* inputproj_dtype codes */
} inputproj_types;

typedef struct inputproj_levels {
    void *p[INPUTPROJ_MAX_LEVELS];      /* one device pointer per level; entries at and beyond L are not read */
} inputproj_levels;

int inputproj_version(void);
const char *inputproj_last_error(void);
int inputproj_tile(int which);          /* -1 for an unknown constant */

/* S = sum_l H_l * W_l; negative on a bad argument.  Host arithmetic only. */
long long inputproj_tokens(const inputproj_shape *shape);

/* Bytes of the workspace of inputproj_forward, a multiple of 256 (0 when every group is one chunk): 2 floats per chunk of
 * every group; negative on a bad argument.  Host arithmetic only. */
long long inputproj_forward_workspace_bytes(const inputproj_shape *shape);

/* Bytes of the workspace of inputproj_backward, a multiple of 256: 2 * C floats per pixel chunk of every frame and level, and
 * 2 floats per group; negative on a bad argument.  Host arithmetic only. */
long long inputproj_backward_workspace_bytes(const inputproj_shape *shape);

/* tokens [N, S, C], mean and rstd [N, L, G] (all three required), every element written: a statistics pass, a combine pass
 * when a group spans several chunks (workspace then required, 16-byte aligned, uninitialised), and the apply pass.  No
 * elements: a no-op. */
int inputproj_forward(const inputproj_types *types, const inputproj_levels *x, const inputproj_levels *weight,
                      const inputproj_levels *bias, double eps, const inputproj_shape *shape, void *workspace, void *tokens,
                      float *mean, float *rstd, void *stream);

/* The gradients whose pointers are given, every element written.  workspace: at least inputproj_backward_workspace_bytes()
 * bytes, 16-byte aligned, uninitialised.  weight_l is required where grad_x_l is given.  All 3 L outputs NULL is an argument
 * error. */
int inputproj_backward(const inputproj_types *types, const inputproj_levels *x, const inputproj_levels *weight, const float *mean,
                       const float *rstd, const void *grad_tokens, const inputproj_shape *shape, void *workspace,
                       const inputproj_levels *grad_x, const inputproj_levels *grad_weight, const inputproj_levels *grad_bias,
                       void *stream);

#ifdef __cplusplus
}
#endif

#endif /* INPUTPROJ_H */
