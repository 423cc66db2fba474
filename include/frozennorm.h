/*
 * frozennorm.h -- C ABI of the glue of the ResNet backbone's blocks in libmsda_hip.so: what the
 * reference's FrozenBatchNorm2d (src/models/backbone.py) and torchvision's Bottleneck / BasicBlock / stem compute between
 * their convolutions -- the frozen norm's affine map, the ReLU, the shortcut add with the downsample branch's norm folded in,
 * and the stem's max-pool -- each as one pass (frozennorm_forward, frozennorm_backward, frozennorm_pool_forward).
 *
 * The rule.  Arithmetic is float for every storage dtype; every operation below is rounded on its own except the fma, which is
 * one fused multiply-add.  For channel c, from the four float32 buffers of a norm and its eps (rounded to float once):
 *     s[c] = weight[c] * (1 / sqrt(var[c] + eps))
 *     t[c] = bias[c] - mean[c] * s[c]
 * computed inside the kernel -- no prologue launch, no cached tensor.  Then per element, with (s1, t1) of `norm` and (s2, t2)
 * of `norm_r`:
 *     v = fma(x, s1[c], t1[c])
 *     FROZENNORM_NONE      z = v
 *     FROZENNORM_PLAIN     z = v + r
 *     FROZENNORM_NORMED    z = v + fma(r, s2[c], t2[c])                  (the block's downsample branch)
 *     y = relu ? (z > 0 ? z : (z == z ? 0 : z)) : z                      (a NaN stays a NaN, as in torch.relu)
 *   y is rounded once, at the store.  This order is the same for every layout, alignment, load width and batch size: an
 *   element's bits depend on its operands and its channel's buffers alone.
 *
 * Backward.  g = float(grad_y), m = relu ? (y > 0) : 1 -- torch's threshold_backward: 0 at y == 0 and at NaN --,
 *     grad_x = (m ? g : 0) * s1[c]
 *     grad_r = (m ? g : 0)              (PLAIN)        (m ? g : 0) * s2[c]       (NORMED)
 *   Each output pointer may be NULL: what is not asked for is not computed.  y is read only when relu is set.  The buffers are
 *   frozen: there are no parameter gradients and no reductions.
 *
 * The stem.  frozennorm_pool_forward: y = max_pool2d(relu(fma(x, s, t)), kernel 3, stride 2, padding 1, dilation 1, floor
 *   mode): output (Ho, Wo) = ((H - 1) / 2 + 1, (W - 1) / 2 + 1) = frozennorm_pooled_size().  Every tap of the window that lies
 *   inside H x W goes through the affine map and the ReLU before the maximum is taken (a negative s reverses the order); the
 *   taps are visited rows ascending, then columns ascending, and a tap replaces the running maximum when it is greater or a
 *   NaN (F.max_pool2d's rule).  The full-resolution normalised map never exists.  Forward only.
 *
 * Layouts.  frozennorm_shape.layout: FROZENNORM_NCHW -- x, r and y are dense [N, C, H, W]: planes of H * W elements whose
 *   constants are wave-uniform -- or FROZENNORM_NHWC -- dense [N, H, W, C] memory (torch's channels-last): rows of C, a lane
 *   keeps the constants of its channels in registers across rows.  x, r and y (and the gradients) share one layout.
 *
 * dtypes.  frozennorm_types names the dtype of x (and grad_x), of r (and grad_r) and of y (and grad_y) among F32, BF16 and
 *   F16, each on its own, with one restriction: BF16 and F16 do not meet in one call.  Without r, types.r must equal types.x.
 *   The buffers are float32.  float64 is not a kernel dtype.
 *
 * Kernels (gfx950, wave64).  16-byte loads and stores when every tensor pointer is 16-byte aligned (and, in NHWC, C is a
 *   multiple of the vector width V -- 4 elements when all three dtypes are F32, 8 otherwise): in NCHW each plane is cut into a
 *   head up to the next 16-byte boundary, a body of vectors and a tail, so planes that are no multiple of V, planes shorter
 *   than V and planes that start off the 16-byte grid are covered.  Otherwise a per-element path that gives the same bits.
 *   (The NCHW pool reads per element.)  No LDS, no atomics, no scratch; every output element is written exactly once.
 *
 * Conventions (those of prenorm.h)
 *   - every pointer is a DEVICE pointer; tensors are dense and need element alignment only;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and never
 *     synchronise (HIP-graph capture works), and are re-entrant;
 *   - element offsets are 64-bit; C, H and W fit 31 bits each and N is a long long;
 *   - return value: FROZENNORM_OK (0) or a negative frozennorm_status; on failure frozennorm_last_error() returns a
 *     thread-local message.  Arguments are checked before any HIP call, so argument errors are reported without a GPU.
 */
#ifndef FROZENNORM_H
#define FROZENNORM_H

#ifdef __cplusplus
extern "C" {
#endif

#define FROZENNORM_ABI_VERSION 1

typedef enum frozennorm_status { FROZENNORM_OK = 0, FROZENNORM_ERR_ARGUMENT = -1, FROZENNORM_ERR_HIP = -2 } frozennorm_status;

/* (code 1, float64 elsewhere in this library, is refused) */
typedef enum frozennorm_dtype { FROZENNORM_F32 = 0, FROZENNORM_BF16 = 2, FROZENNORM_F16 = 3 } frozennorm_dtype;

typedef enum frozennorm_layout { FROZENNORM_NCHW = 0, FROZENNORM_NHWC = 1 } frozennorm_layout;

typedef enum frozennorm_residual { FROZENNORM_NONE = 0, FROZENNORM_PLAIN = 1, FROZENNORM_NORMED = 2 } frozennorm_residual;

typedef struct frozennorm_shape {
    long long N;            /* batch entries */
    int C, H, W;            /* channels and the map of x (the pool's output is smaller) */
    int layout;             /* frozennorm_layout */
    int residual;           /* frozennorm_residual */
    int relu;               /* 0 or 1 (the pool always applies it) */
} frozennorm_shape;

typedef struct frozennorm_types {
    int x, r, y;            /* frozennorm_dtype codes */
} frozennorm_types;

/* the four float32 buffers [C] of a frozen norm and its eps */
typedef struct frozennorm_norm {
    const float *weight, *bias, *mean, *var;
    double eps;
} frozennorm_norm;

int frozennorm_version(void);
const char *frozennorm_last_error(void);

/* The pool's output extent for an input extent n: (n - 1) / 2 + 1, 0 for 0, -1 for a negative n. */
int frozennorm_pooled_size(int n);

/* y, every element written, in one enqueued pass.  r is required in PLAIN and NORMED and must be NULL in NONE; norm_r is
 * required in NORMED and must be NULL otherwise.  A call without elements is a no-op that dereferences nothing. */
int frozennorm_forward(const frozennorm_types *types, const frozennorm_shape *shape, const void *x, const frozennorm_norm *norm,
                       const void *r, const frozennorm_norm *norm_r, void *y, void *stream);

/* The gradients that are given, every element written, in one enqueued pass.  y (the forward's output) is required when
 * shape->relu is set and not read otherwise; norm (weight, var and eps are read) is required for grad_x, norm_r for grad_r in
 * NORMED.  grad_r may be given in PLAIN and NORMED only.  Both outputs NULL is an argument error. */
int frozennorm_backward(const frozennorm_types *types, const frozennorm_shape *shape, const void *grad_y, const void *y,
                        const frozennorm_norm *norm, const frozennorm_norm *norm_r, void *grad_x, void *grad_r, void *stream);

/* y [N, C, Ho, Wo] (in the shape's layout), every element written, in one enqueued pass.  shape->residual must be NONE;
 * types->r must equal types->x. */
int frozennorm_pool_forward(const frozennorm_types *types, const frozennorm_shape *shape, const void *x,
                            const frozennorm_norm *norm, void *y, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FROZENNORM_H */
