/*
 * swinends.h -- C ABI of the two ends of the Swin backbone in libmsda_hip.so: what the reference's
 * PatchEmbed.forward and the per-stage output norms of SwinTransformer.forward (src/models/swin_backbone.py) compute around
 * the blocks -- the zero padding, the p x p / stride-p projection and its LayerNorm written straight into token order
 * (swinends_embed_*), and the LayerNorm of a stage's tokens written straight into the NCHW map (swinends_map_*).
 *
 * ---- swinends_embed: image [B, Cin, H, W] -> tokens [B * Hp * Wp, C] ----------------------------------------------------------
 * Hp = ceil(H / p), Wp = ceil(W / p); token n = (b * Hp + i) * Wp + j.  K = Cin * p * p, 1 <= K <= SWINENDS_MAX_PATCH;
 * 1 <= C <= SWINENDS_MAX_EMBED.  A is float for every storage dtype.
 *   patch[k], k = (cin * p + dy) * p + dx (proj_weight's memory order, proj_weight being [C, Cin, p, p] = [C, K]):
 *       A(image[b, cin, i * p + dy, j * p + dx]), and exactly 0 where that pixel lies outside H x W -- the reference's right
 *       and bottom zero padding; no padded image exists.
 *   The projection: acc = 0; for k = 0 .. K - 1 ascending: acc = fma(A(proj_weight[c, k]), patch[k], acc) (one rounding per
 *       step); z[c] = acc + A(proj_bias[c]) (proj_bias NULL: z = acc).  On the VALU.  The chain of a token depends on K alone:
 *       its bits do not depend on B, on the image it lies in, on where it falls in a tile, on the alignment of the operands or
 *       on the launch geometry.
 *   The norm (norm_weight and norm_bias both given): prenorm.h's "The norm" paragraph over z (which is NOT rounded to a storage
 *       dtype first), with prenorm.h's order of the sums over C:
 *           mean = sum_c(z) / C, var = sum_c((z - mean)^2) / C, rstd = 1 / sqrt(var + eps),
 *           tokens = ((z - mean) * rstd) * norm_weight + norm_bias, rounded once at the store.
 *       mean and rstd [B * Hp * Wp], float32, are written when given.  Both NULL (patch_norm=False): tokens = z, rounded once.
 *   Backward.  Nothing of token size is kept: z is computed again from the image, by the same chain (the same bits).  With
 *   g = A(grad_tokens), xhat = (z - mean) * rstd from the saved statistics, gw = g * norm_weight:
 *           c1 = sum_c(gw) / C, c2 = sum_c(gw * xhat) / C, dz = ((gw - c1) - xhat * c2) * rstd        (without a norm: dz = g)
 *           grad_norm_weight[c] = sum_n(g * xhat), grad_norm_bias[c] = sum_n(g), grad_proj_bias[c] = sum_n(dz)
 *           grad_proj_weight[c, k] = sum_n(dz[c] * patch[k])
 *       A gradient of the image is not computed.  Order of the sums over the tokens: tokens are cut into chunks of
 *       swinends_tile(SWINENDS_TILE_EMBED_CHUNK) consecutive tokens, a chunk into tiles of swinends_tile(SWINENDS_TILE_TOKENS).
 *       Column sums of a chunk: wave w (0..3) of the chunk's workgroup adds the tokens 8 w .. 8 w + 7 of every tile, tiles and
 *       tokens ascending; the four waves are added ascending.  grad_proj_weight of a chunk: per tile the chain
 *       s = 0, s = fma(dz[t, c], patch[t, k], s) over the tile's tokens ascending, the tiles' sums added ascending into the
 *       chunk's partial (by the one thread that owns the element: no atomics).  The chunks' partials lie in the workspace and a
 *       combine launch adds them as prenorm.h's does: lane l of a wave adds the chunks l, l + 64, .. ascending, butterflies
 *       (xor 32 .. 1), rounded once to the parameters' dtype.  Two enqueued passes.  No [tokens, K] tensor exists.
 *   dtypes (swinends_embed_types: image, param = all four parameters and their gradients, y = tokens and grad_tokens): one of
 *       F32 / BF16 / F16 for all three; or F32 image and parameters beside a 16-bit y.
 *
 * ---- swinends_map: x [B, H * W, C] -> y [B, C, H, W] ---------------------------------------------------------------------------
 * 1 <= C <= SWINENDS_MAX_CHANNELS.  y[b, c, h, w] = LayerNorm(x[b, h * W + w, :])[c]: the row arithmetic and the order of the sums
 * over C are prenorm_forward's PRENORM_PLAIN / PRENORM_TOKENS (the same device code), so y is bit for bit that call's y,
 * permuted; mean and rstd [B * H * W] likewise.  Backward: grad_y [B, C, H, W]; grad_x [B, H * W, C] by prenorm.h's dz formula
 * (grad_s = 0) with the saved mean and rstd, bit for bit prenorm_backward's.  grad_weight[c] = sum_r(g * xhat),
 * grad_bias[c] = sum_r(g): rows are cut into chunks of swinends_tile(SWINENDS_TILE_TOKENS) consecutive rows; wave w of the
 * chunk's workgroup adds the rows 8 w .. 8 w + 7 ascending, the four waves are added ascending, and the chunks are combined as
 * above.  Each output pointer of a backward may be NULL: what is not asked for is not computed.
 *   dtypes (swinends_map_types: x and grad_x, y and grad_y, param): one dtype for all; F32 x and parameters beside a 16-bit y;
 *   F32 parameters beside 16-bit x and y.
 *
 * Kernels (gfx950, wave64, 256 threads).  A workgroup owns a tile of 32 consecutive tokens (of the whole batch: a tile may span
 * batch entries, the last one is partial); a wave owns 8 of them and holds a row in registers.  embed: the tile's patches lie
 * in LDS as [K][32], the projection weight is staged through LDS in slices of k, transposed to [k][C] so that a lane reads its
 * four channels in one access.  map: normalised rows are deposited in an LDS tile [256 channels][32 tokens], row pitch 33
 * floats, channel 4 l + j of a group at tile row 64 j + l (deposits and reads are free of bank conflicts), and written --
 * backward: read -- along the tokens, 128-byte runs per channel; rows of more than 256 channels take one pass per 256.
 * No float atomics, nothing is zeroed by a pass of its own: every output element is written by the launch that owns it.
 *
 * Conventions (those of prenorm.h)
 *   - every pointer is a DEVICE pointer; tensors are dense and need element alignment only;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and never
 *     synchronise (HIP-graph capture works), and are re-entrant;
 *   - element offsets are 64-bit; the number of tokens must fit 31 bits;
 *   - return value: SWINENDS_OK (0) or a negative swinends_status; on failure swinends_last_error() returns a thread-local
 *     message.  Arguments are checked before any HIP call, so argument errors are reported without a GPU.
 */
#ifndef SWINENDS_H
#define SWINENDS_H

#ifdef __cplusplus
extern "C" {
#endif

#define SWINENDS_ABI_VERSION 1

typedef enum swinends_status { SWINENDS_OK = 0, SWINENDS_ERR_ARGUMENT = -1, SWINENDS_ERR_HIP = -2 } swinends_status;

/* (code 1, float64 elsewhere in this library, is refused) */
typedef enum swinends_dtype { SWINENDS_F32 = 0, SWINENDS_BF16 = 2, SWINENDS_F16 = 3 } swinends_dtype;

#define SWINENDS_MAX_PATCH 192          /* K = Cin * p * p of the embedding */
#define SWINENDS_MAX_EMBED 1024         /* C of the embedding */
#define SWINENDS_MAX_CHANNELS 3072      /* C of the output norm: PRENORM_MAX_CHANNELS */

/* swinends_tile(): which constant of the kernels' tiling */
#define SWINENDS_TILE_TOKENS 0          /* tokens of a workgroup's tile; rows of a chunk of the map backward's column sums */
#define SWINENDS_TILE_EMBED_CHUNK 1     /* tokens of a chunk of the embedding backward's sums */
#define SWINENDS_TILE_MAX_PATCH 2       /* SWINENDS_MAX_PATCH */
#define SWINENDS_TILE_MAX_EMBED 3       /* SWINENDS_MAX_EMBED */
#define SWINENDS_TILE_MAX_CHANNELS 4    /* SWINENDS_MAX_CHANNELS */

typedef struct swinends_embed_shape {
    long long B;            /* images */
    int Cin, H, W;          /* channels and size of an image */
    int p;                  /* the patch is p x p, stride p */
    int C;                  /* embedding channels */
} swinends_embed_shape;

typedef struct swinends_embed_types {
    int image, param, y;    /* swinends_dtype codes */
} swinends_embed_types;

typedef struct swinends_map_shape {
    long long B;
    int H, W, C;
} swinends_map_shape;

typedef struct swinends_map_types {
    int x, y, param;        /* swinends_dtype codes */
} swinends_map_types;

int swinends_version(void);
const char *swinends_last_error(void);
int swinends_tile(int which);       /* -1 for an unknown constant */

/* Tokens B * Hp * Wp of a shape; negative on a bad argument.  Host arithmetic only. */
long long swinends_embed_tokens(const swinends_embed_shape *shape);

/* Bytes of the workspace of swinends_embed_backward, a multiple of 256; negative on a bad argument: chunks * 3 * C floats,
 * and chunks * K * C more when `want_weight` (grad_proj_weight will be asked for).  Host arithmetic only. */
long long swinends_embed_workspace_bytes(const swinends_embed_shape *shape, int want_weight);

/* tokens, every element written, in one enqueued pass; mean and rstd when given (both or neither; only with a norm).
 * proj_bias may be NULL; norm_weight and norm_bias are given together or not at all.  No tokens: a no-op. */
int swinends_embed_forward(const swinends_embed_types *types, const void *image, const void *proj_weight, const void *proj_bias,
                           const void *norm_weight, const void *norm_bias, double eps, const swinends_embed_shape *shape,
                           void *tokens, float *mean, float *rstd, void *stream);

/* The gradients that are given, every element written, in two enqueued passes.  norm_weight, mean and rstd are given together
 * (the forward had a norm) or not at all; grad_norm_weight and grad_norm_bias only with them.  workspace: at least
 * swinends_embed_workspace_bytes() bytes, 16-byte aligned, uninitialised.  All four outputs NULL is an argument error. */
int swinends_embed_backward(const swinends_embed_types *types, const void *image, const void *proj_weight, const void *proj_bias,
                            const void *norm_weight, const float *mean, const float *rstd, const void *grad_tokens,
                            const swinends_embed_shape *shape, void *workspace, void *grad_proj_weight, void *grad_proj_bias,
                            void *grad_norm_weight, void *grad_norm_bias, void *stream);

/* Bytes of the workspace of swinends_map_backward when grad_weight or grad_bias is asked for, a multiple of 256: chunks * 2 * C
 * floats; negative on a bad argument.  Host arithmetic only. */
long long swinends_map_workspace_bytes(const swinends_map_shape *shape);

/* y [B, C, H, W], every element written, in one enqueued pass; mean and rstd [B * H * W] when given (both or neither). */
int swinends_map_forward(const swinends_map_types *types, const void *x, const void *weight, const void *bias, double eps,
                         const swinends_map_shape *shape, void *y, float *mean, float *rstd, void *stream);

/* The gradients that are given, every element written: one enqueued pass, and a combine pass when grad_weight or grad_bias is
 * given (workspace then required, 16-byte aligned, uninitialised).  All three outputs NULL is an argument error. */
int swinends_map_backward(const swinends_map_types *types, const void *x, const void *weight, const float *mean, const float *rstd,
                          const void *grad_y, const swinends_map_shape *shape, void *workspace, void *grad_x, void *grad_weight,
                          void *grad_bias, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SWINENDS_H */
