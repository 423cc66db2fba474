/*
 * posembed.h -- C ABI of the encoder's positional input in libmsda_hip.so: what DeVIS's
 * PositionEmbeddingSine / PositionEmbeddingSineWithLearnableTemporal, the `.to(dtype)` of their callers and the positional part
 * of DeformableTransformer.prepare_data compute from the padding masks -- the sine embedding of every token plus the temporal
 * and the level embedding, written once in the layout the encoder reads, together with the flattened masks and the valid
 * ratios -- and the gradient of the two embeddings.
 *
 * Geometry: N frames, L <= POSEMBED_MAX_LEVELS levels of H[l] x W[l] pixels, C = 2 * F channels (F = num_pos_feats, even).
 * S = sum_l H[l] * W[l] tokens per frame; level l starts at token start[l] = sum_{k < l} H[k] * W[k]; token start[l] + y * W[l]
 * + x is pixel (y, x).  A mask is bool / uint8 [N, H[l], W[l]] with ELEMENT strides (sn, sy, sx): nonzero is padding.
 *
 * Definition (the reference's float32 operations in the reference's order; v = !mask)
 *   cy[n, y, x] = sum_{y' <= y} v[n, y', x]        cx[n, y, x] = sum_{x' <= x} v[n, y, x']        (integers: cumsum)
 *   ty[n, x]    = cy[n, H-1, x]                    tx[n, y]    = cx[n, y, W-1]                    (the totals)
 *   ey = normalize ? (float)cy / ((float)ty + 1e-6f) * scale : (float)cy          and ex alike from cx, tx
 *   for k in [0, F):  a = e / dim_t[k];   sine[k] = k even ? sinf(a) : cosf(a)     (dim_t[k] == dim_t[k ^ 1]: one sincosf a pair)
 *   channel c < F is sine_y[c], channel c >= F is sine_x[c - F]                    (the y half before the x half)
 *   flat:  v = sine + temporal_embed[n, c]   (when given);   v = round(v) to round_dtype (when given);
 *          pos[n, start[l] + y * W + x, c] = v + level_embed[l, c]                 (one rounding at the store)
 *   nchw:  pos[n, c, y, x] = sine                                                  (one level, no embeddings)
 *   mask_flatten[n, start[l] + y * W + x] = mask byte != 0
 *   valid_ratios[n, l] = ((float)tx[n, 0] * (1.0f / (float)W), (float)ty[n, 0] * (1.0f / (float)H))
 *                        the reference's order (w, h), and its float32 division AS IT RUNS ON THE DEVICE: torch divides a
 *                        device tensor by a host scalar by multiplying with the scalar's float32 reciprocal, which can differ
 *                        from the quotient (what torch computes on the CPU) in the last bit
 * dim_t is an OPERAND, float32 [F]: the caller builds the reference's table with the reference's expression, so that it is
 * that table bit for bit.  sinf / cosf are the accurate ones, not the fast intrinsics.  Arithmetic is float32, every
 * operation rounded on its own (no fused multiply-add).
 *
 *   Backward of the flat layout: the differentiable operands are level_embed [L, C] and temporal_embed [N, C] alone.
 *     S[n, l, c]             = sum over the tokens of level l of grad[n, token, c]
 *     grad_level_embed[l]    = sum_n S[n, l]            grad_temporal_embed[n] = sum_l S[n, l]
 *   (with round_dtype the rounding is treated as the identity, as autograd treats `.to(dtype)`.)  Order: a level's tokens are
 *   cut into chunks of posembed_tile(POSEMBED_TILE_TOKENS) counted from the level's own start; inside a chunk a workgroup's
 *   four waves take the tokens w, w + 4, ... ascending and are added ascending; S adds its chunks ascending; grad_level_embed
 *   adds n ascending; grad_temporal_embed adds the levels in the order of DESCENDING H * W, then H, then position in the call.
 *   No atomics: the gradients are bitwise reproducible, and do not depend on the order of the levels in the call as long as
 *   no two levels have the same H and W.  Either gradient pointer may be NULL: it is then not computed.
 *
 * Kernels
 *   counts   one launch for all frames and levels.  Row workgroups: one wave per row; a lane per pixel of a 64-pixel chunk,
 *            wave ballot and popcount, the count CARRIED from chunk to chunk, so any W is right; they also copy the mask
 *            bytes to mask_flatten, and the wave of row 0 writes valid_ratios[n, l, 0].  Column workgroups: a lane per
 *            column walking down the rows; the lane of column 0 writes valid_ratios[n, l, 1].  Results: cy, cx int32 [N, S],
 *            ty int32 [N, sum W], tx int32 [N, sum H] in the workspace, in this order, each region 256-byte aligned.
 *   write    one launch.  flat: the output is one dense array of N * S * C elements; a lane owns 16 bytes of it (4 float32,
 *            8 16-bit elements) and stores them with one 16-byte store -- lanes run along channels --, and the last
 *            N * S * C mod (elements of 16 bytes) elements are a scalar tail.  nchw: a lane per (n, pair of channels, y, x),
 *            lanes along x.
 *   backward a partial pass (one workgroup per frame, chunk and 64 channels) into the workspace and a combine pass.
 *
 * Conventions (those of labelloss.h)
 *   - every pointer is a DEVICE pointer; `pos` must be 16-byte aligned, the others need element alignment only;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and never
 *     synchronise (HIP-graph capture works), and are re-entrant;
 *   - element offsets are 64-bit; N * S and C must fit 31 bits;
 *   - return value: POSEMBED_OK (0) or a negative posembed_status; on failure posembed_last_error() returns a thread-local
 *     message.  Arguments are checked before any HIP call, so argument errors are reported without a GPU.
 */
#ifndef POSEMBED_H
#define POSEMBED_H

#ifdef __cplusplus
extern "C" {
#endif

#define POSEMBED_ABI_VERSION 1
#define POSEMBED_MAX_LEVELS 8

typedef enum posembed_status { POSEMBED_OK = 0, POSEMBED_ERR_ARGUMENT = -1, POSEMBED_ERR_HIP = -2 } posembed_status;

/* the output dtype; POSEMBED_F64 is declared for the shared numbering and refused */
typedef enum posembed_dtype { POSEMBED_F32 = 0, POSEMBED_F64 = 1, POSEMBED_BF16 = 2, POSEMBED_F16 = 3 } posembed_dtype;
#define POSEMBED_NO_ROUNDING (-1)   /* round_dtype: none */

/* posembed_tile(): which constant of the kernels' tiling */
#define POSEMBED_TILE_TOKENS 0      /* tokens of one level and frame per workgroup of the backward's partial pass */
#define POSEMBED_TILE_CHANNELS 1    /* channels per workgroup of the backward's partial pass */
#define POSEMBED_TILE_PIXELS 2      /* pixels of a row a wave of the counts pass takes at a time */

/* posembed_workspace_bytes(): for which call */
#define POSEMBED_WS_COUNTS 0
#define POSEMBED_WS_BACKWARD 1

typedef struct posembed_shape {
    int N, L, C;                            /* frames, levels, channels (C = 2 * num_pos_feats) */
    int H[POSEMBED_MAX_LEVELS], W[POSEMBED_MAX_LEVELS];
} posembed_shape;

typedef struct posembed_masks {
    const unsigned char *ptr[POSEMBED_MAX_LEVELS];
    long long sn[POSEMBED_MAX_LEVELS], sy[POSEMBED_MAX_LEVELS], sx[POSEMBED_MAX_LEVELS];      /* element strides */
} posembed_masks;

int posembed_version(void);
const char *posembed_last_error(void);
int posembed_tile(int which);       /* -1 for an unknown constant */

/* Bytes of the workspace of posembed_counts (which the write passes read) or of posembed_backward, a multiple of 256;
 * negative on a bad argument.  Host arithmetic only. */
long long posembed_workspace_bytes(int which, const posembed_shape *shape);

/* The counts pass: the workspace (at least posembed_workspace_bytes(POSEMBED_WS_COUNTS) bytes, 16-byte aligned,
 * uninitialised), mask_flatten [N, S] bytes and valid_ratios [N, L, 2] float32, every word written.  mask_flatten and
 * valid_ratios may be NULL: they are then not written.  `C` of the shape is not read.  N * S == 0 is a no-op. */
int posembed_counts(const posembed_masks *masks, const posembed_shape *shape, void *workspace, unsigned char *mask_flatten,
                    float *valid_ratios, void *stream);

/* The write pass, flat layout: pos [N, S, C] in `dtype`, every element written, from the workspace posembed_counts left.
 * dim_t float32 [C / 2]; level_embed float32 [L, C]; temporal_embed float32 [N, C] or NULL; round_dtype POSEMBED_BF16,
 * POSEMBED_F16 or POSEMBED_NO_ROUNDING; `scale` is read when `normalize` is nonzero. */
int posembed_write_flat(int dtype, const void *workspace, const posembed_shape *shape, const float *dim_t,
                        const float *level_embed, const float *temporal_embed, int normalize, float scale, int round_dtype,
                        void *pos, void *stream);

/* The write pass, nchw layout: pos [N, C, H[0], W[0]] in `dtype` of a shape with L == 1. */
int posembed_write_nchw(int dtype, const void *workspace, const posembed_shape *shape, const float *dim_t, int normalize,
                        float scale, void *pos, void *stream);

/* grad_level_embed float32 [L, C] and grad_temporal_embed float32 [N, C] (either may be NULL, not both) from grad [N, S, C]
 * in `dtype`; workspace: at least posembed_workspace_bytes(POSEMBED_WS_BACKWARD) bytes, uninitialised.  Two enqueued passes.
 * With N * S == 0 the requested gradients are written as zeros by the combine pass alone. */
int posembed_backward(int dtype, const void *grad, const posembed_shape *shape, void *workspace, float *grad_level_embed,
                      float *grad_temporal_embed, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* POSEMBED_H */
