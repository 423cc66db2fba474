/*
 * mhstage.h -- C ABI of one stage of the mask head's glue (DeVIS MaskHeadConv, between two of its convolutions) in
 * libmsda_hip.so: GroupNorm, ReLU, nearest-neighbour upsampling, the FPN add and the concatenation of the attention
 * maps, fused into one statistics pass and one apply pass that writes the result once, channels-last (DESIGN.md
 * section 10).
 *
 * Geometry: N images of C channels in G groups on an h x w map; F skip images of C channels and N images of E extra
 * channels on the H x W output map.  p = h*w, P = H*W, g(c) = c / (C/G).
 *
 *   mean[n,g], var[n,g] = mean and biased variance of x[n, the channels of g, :]
 *   rstd[n,g]    = 1 / sqrt(var + eps)
 *   xhat[n,c,s]  = (x[n,c,s] - mean[n,g(c)]) * rstd[n,g(c)]
 *   z[n,c,s]     = xhat * weight[c] + bias[c]                        (one fused multiply-add)
 *   y[n,c,s]     = z > 0 ? z : 0                                     (NaN stays NaN)
 *   out[n,c,d]   = y[n,c,src(d)] + skip[skip_index[n], c, d]         c < C      (without skip: y alone)
 *   out[n,C+e,d] = extra[n,e,d]                                      e < E
 *
 * src is PyTorch's mode="nearest" rule, per axis, evaluated in float32 for every dtype:
 *
 *   src(d) = min((int)floorf((float)d * ((float)h / (float)H)), h - 1)          (w and W for columns)
 *
 * (not the integer rule (d * h) / H, which differs, e.g. for 14 -> 46 at d = 23).  With H == h it is the identity.
 * The variance is a sum of squared deviations from the mean (per tile, tiles combined by the parallel-variance
 * formula), never E[x^2] - mean^2.
 *
 * Backward.  With g[n,c,s] = the sum of grad_out[n,c,d] over the d with src(d) = s (a contiguous range per axis, summed
 * rows first, columns ascending), dy = g where z > 0 (strictly; z recomputed by the forward's expression) else 0, and
 * m = (C/G) * p:
 *   S1[n,g] = sum over the group of weight*dy        S2[n,g] = sum over the group of weight*dy*xhat
 *   grad_x      = rstd * (weight*dy - S1/m - xhat * S2/m)
 *   grad_weight = sum over n, s of dy*xhat           grad_bias = sum over n, s of dy
 *   grad_skip[f] = sum over the n with skip_index[n] == f, ascending, of grad_out[n, :C]
 * grad_extra is the slice grad_out[:, C:] and is the caller's.  There are no float atomics anywhere: every sum has a
 * fixed order (butterflies within a wave, fixed-order loops over waves, tiles and images), so every result is bitwise
 * reproducible, an image has the same bits alone and in a batch, and a gradient computed alone has the bits it has in
 * a full backward.
 *
 * Conventions (those of attmap.h)
 *   - every pointer is a DEVICE pointer unless stated; tensors are dense:
 *       x [N, C, h, w] and skip [F, C, H, W] and extra [N, E, H, W] in NCHW; weight, bias [C]; mean, rstd [N, G];
 *       out [N, H, W, C+E] (channels-last memory of the logical [N, C+E, H, W]);
 *       grad_out: logical [N, C+E, H, W] in NCHW memory (layout 0) or in channels-last memory (layout 1);
 *       skip_index [N] int32 (index_is64 == 0) or int64, or NULL for the identity (then F == N);
 *   - skip_index values outside [0, F) are the caller's contract: the library does not read device memory on the host
 *     and cannot check them; such a value reads or skips out of bounds;
 *   - `dtype` is an mhstage_dtype: the storage type of x, skip, grad_x and grad_skip.  The `*_wide` flags say that the
 *     tensor they name is float32 beside a 16-bit `dtype` (they must be 0 beside MHSTAGE_F32 / MHSTAGE_F64):
 *     param_wide weight, bias, grad_weight, grad_bias; extra_wide extra; out_wide out and grad_out.
 *     mean, rstd, the dy buffer and the workspace hold the arithmetic type: float, double for MHSTAGE_F64;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and
 *     never synchronise (HIP-graph capture works), and are re-entrant;
 *   - element offsets are 64-bit; p, P, C+E and (C/G)*p must fit 31 bits;
 *   - return value: MHSTAGE_OK (0) or a negative mhstage_status; on failure mhstage_last_error() returns a
 *     thread-local message.  Arguments are checked before any HIP call, so argument errors are reported without a GPU.
 */
#ifndef MHSTAGE_H
#define MHSTAGE_H

#ifdef __cplusplus
extern "C" {
#endif

#define MHSTAGE_ABI_VERSION 1

typedef enum mhstage_status { MHSTAGE_OK = 0, MHSTAGE_ERR_ARGUMENT = -1, MHSTAGE_ERR_HIP = -2 } mhstage_status;

typedef enum mhstage_dtype { MHSTAGE_F32 = 0, MHSTAGE_F64 = 1, MHSTAGE_BF16 = 2, MHSTAGE_F16 = 3 } mhstage_dtype;

/* which gradients mhstage_backward computes */
#define MHSTAGE_GRAD_X 1
#define MHSTAGE_GRAD_WEIGHT 2
#define MHSTAGE_GRAD_BIAS 4
#define MHSTAGE_GRAD_SKIP 8

/* mhstage_tile(): which constant of the kernels' tiling */
#define MHSTAGE_TILE_STAT 0         /* elements of a group block per statistics tile */
#define MHSTAGE_TILE_APPLY_PIXELS 1 /* destination pixels per workgroup of the apply pass */
#define MHSTAGE_TILE_APPLY_CHANNELS 2
#define MHSTAGE_TILE_BWD_PIXELS 3   /* source pixels per workgroup of backward pass 1 */

typedef struct mhstage_shape {
    int N, F, C, G, E, h, w, H, W;  /* F is read only with a skip; without skip and extra (H, W) must be (h, w) */
} mhstage_shape;

int mhstage_version(void);
const char *mhstage_last_error(void);
int mhstage_tile(int which);        /* -1 for an unknown constant */

/* Bytes of the workspace of mhstage_forward and of mhstage_backward (the larger of the two), a multiple of 256;
 * negative on a bad argument.  Forward: two arithmetic values per (image, group, statistics tile).  Backward: two per
 * (image, channel, source-pixel tile), two per (image, channel) and two per (image, group).  Host arithmetic only. */
long long mhstage_workspace_bytes(int dtype, const mhstage_shape *shape);

/* mean, rstd and out, in two or three enqueued passes:
 *   statistics  per (image, group, tile) the tile's mean and sum of squared deviations; a group block of one tile
 *               writes mean and rstd at once, otherwise a second launch combines the tiles in a fixed order;
 *   apply       per (image, 32 channels, 64 destination pixels): gather at src(d), normalise, gate, add the skip,
 *               transpose through LDS, write channel-contiguous rows; extra's channels go to the row tail.
 * skip (with F, skip_index) and extra may be NULL.  out, mean and rstd are written exactly once, every element.
 * workspace: at least mhstage_workspace_bytes() bytes, 16-byte aligned, uninitialised.  N == 0 is a no-op. */
int mhstage_forward(int dtype, int param_wide, int extra_wide, int out_wide, const void *x, const void *weight,
                    const void *bias, double eps, const void *skip, const void *skip_index, int index_is64,
                    const void *extra, const mhstage_shape *shape, void *workspace, void *mean, void *rstd, void *out,
                    void *stream);

/* The gradients in `grads` (a mask of MHSTAGE_GRAD_*; 0 is a no-op); pointers of gradients not asked for may be NULL.
 *   pass 1   (X, WEIGHT or BIAS) per (image, 16 channels, 256 source pixels): gather g from grad_out, gate it, write
 *            dy [N, C, h, w] in the arithmetic type, and the tile's sums of dy and dy*xhat -> workspace;
 *   combine  per (image, group): the tiles of each channel and the group's S1, S2, in a fixed order;
 *   pass 2   (X) grad_x in `dtype`; it may alias dy when `dtype` is MHSTAGE_F32 or MHSTAGE_F64;
 *   weights  (WEIGHT or BIAS) both sums over the images in a fixed order, in weight's storage type;
 *   skip     (SKIP) grad_skip [F, C, H, W] in `dtype`, every element written (zero for an f no image uses).
 * grad_out_layout: 0 NCHW, 1 channels-last.  E is needed for grad_out's strides; extra itself is not read. */
int mhstage_backward(int grads, int dtype, int param_wide, int out_wide, const void *x, const void *weight,
                     const void *bias, const void *mean, const void *rstd, const void *skip_index, int index_is64,
                     const void *grad_out, int grad_out_layout, const mhstage_shape *shape, void *workspace, void *dy,
                     void *grad_x, void *grad_weight, void *grad_bias, void *grad_skip, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MHSTAGE_H */
