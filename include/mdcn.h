/*
 * mdcn.h -- C ABI of the modulated deformable 2-D convolution (DCNv2; DCNv1 without a mask) in libmsda_hip.so:
 * the native operator of DeVIS's mask head (ModulatedDeformableConv2d, whose forward is one deform_conv2d call).
 *
 * The library holds the two kernels that are not a GEMM; the caller multiplies by the weights:
 *
 *   forward    mdcn_im2col   input, offset, mask -> columns [pixels, K*C]          out          = columns @ weight^T (+ bias)
 *   backward   (caller)      grad_columns [pixels, K*C] = grad_out @ weight        grad_weight  = grad_out^T @ columns
 *              mdcn_backward grad_columns, input, offset, mask -> grad_offset, grad_mask, and grad_input (accumulated)
 *              mdcn_backward_input_fixed   grad_columns, offset, mask -> grad_input as an order-independent fixed-point sum
 *
 * Semantics (those of torchvision.ops.deform_conv2d, one weight group): tap k = i*Kw + j of output pixel (ho, wo)
 * samples channel c (offset group g = c / (C/G)) at
 *     y = ho*sh - ph + i*dh + offset[n, 2*(g*K + k),     ho, wo]
 *     x = wo*sw - pw + j*dw + offset[n, 2*(g*K + k) + 1, ho, wo]
 * bilinearly from the input extended by zeros in every direction, times mask[n, g*K + k, ho, wo] (1 without a mask):
 *     columns[(n*Ho + ho)*Wo + wo, k*C + c] = mask * bilinear(input[n, :, :, c], y, x).
 * A point with y <= -1, y >= H, x <= -1 or x >= W samples zero and has zero gradients.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless stated; tensors are dense in the layouts named at each entry point;
 *   - `input` is CHANNELS-LAST, [N, H, W, C]: the four corners of a tap are contiguous channel rows;
 *   - `offset` [N, 2*G*K, Ho, Wo] and `mask` [N, G*K, Ho, Wo] are the caller's NCHW tensors as they stand;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and
 *     never synchronise (HIP-graph capture works), and are re-entrant;
 *   - `dtype` is an mdcn_dtype: the storage type of input / columns / grad_columns and of offset / mask and their
 *     gradients (float beside a 16-bit input for the two *_OFF32 codes).  Arithmetic is fp32, fp64 for MDCN_F64;
 *   - return value: MDCN_OK (0) or a negative mdcn_status; on failure mdcn_last_error() returns a thread-local
 *     message.  Arguments are checked before any HIP call, so argument errors are reported without a GPU.
 */
#ifndef MDCN_H
#define MDCN_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDCN_ABI_VERSION 2

typedef enum mdcn_status { MDCN_OK = 0, MDCN_ERR_ARGUMENT = -1, MDCN_ERR_HIP = -2 } mdcn_status;

typedef enum mdcn_dtype {
    MDCN_F32 = 0, MDCN_F64 = 1, MDCN_BF16 = 2, MDCN_F16 = 3,
    MDCN_BF16_OFF32 = 4,    /* bf16 input / columns, float offset / mask (and their gradients) */
    MDCN_F16_OFF32 = 5      /* f16  input / columns, float offset / mask (and their gradients) */
} mdcn_dtype;

/* gradient groups of mdcn_backward */
#define MDCN_GRAD_INPUT 1       /* grad_input_acc += ... (float atomics: the order of the sum is not fixed) */
#define MDCN_GRAD_SAMPLING 2    /* grad_offset and, with a mask, grad_mask: fully written, bitwise reproducible */

/* One call's geometry.  N is the number of images of THIS call (a batch chunk); Ho, Wo must be the convolution's
 * output size for H, W and the kernel / stride / padding / dilation given; G offset groups, C % G == 0. */
typedef struct mdcn_shape {
    int N, C, H, W, Ho, Wo;
    int Kh, Kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, G;
} mdcn_shape;

int mdcn_version(void);
const char *mdcn_last_error(void);

/* Bytes of the column buffer [batch*Ho*Wo, Kh*Kw*C] of `batch` images in dtype's storage type; negative on a bad
 * argument.  (shape->N is ignored.)  Host arithmetic only. */
long long mdcn_workspace_bytes(int dtype, const mdcn_shape *shape, int batch);

/* Deformable im2col.  input [N, H, W, C], offset, mask (NULL: no modulation) -> columns [N*Ho*Wo, Kh*Kw*C], fully
 * written.  N == 0 is a no-op. */
int mdcn_im2col(int dtype, const void *input, const void *offset, const void *mask, const mdcn_shape *shape,
                void *columns, void *stream);

/* Backward of mdcn_im2col for the gradient groups in `grads`.
 *   grad_columns   [N*Ho*Wo, Kh*Kw*C], storage type;
 *   grad_input_acc [N, H, W, C] in the ARITHMETIC type (float; double for MDCN_F64), ACCUMULATED into with float
 *                  atomics (the caller zeroes it and rounds to the storage type once, after the last chunk); only
 *                  elements inside [0, H) x [0, W) are touched.  Read only with MDCN_GRAD_INPUT;
 *   grad_offset    [N, 2*G*K, Ho, Wo], grad_mask [N, G*K, Ho, Wo] (NULL iff mask is NULL), offset's type, fully written.
 *                  Read only with MDCN_GRAD_SAMPLING. */
int mdcn_backward(int grads, int dtype, const void *input, const void *offset, const void *mask,
                  const void *grad_columns, const mdcn_shape *shape, void *grad_input_acc, void *grad_offset,
                  void *grad_mask, void *stream);

/* ---- order-independent grad_input ---------------------------------------------------------------------------------
 * mdcn_backward's grad_input is a sum of float atomics: its last bits depend on the order the adds arrive in.  The entry
 * below computes the same sum so that every element depends only on the multiset of its terms.
 *
 * The term of (image n, output pixel (ho, wo), tap k, corner q, channel c of offset group g) is
 *     t = (grad_columns[pix, k*C + c] * mask[n, g*K + k, ho, wo]) * w_q
 * evaluated left to right in the arithmetic type with round-to-nearest products and no contraction (without a mask the
 * first factor is grad_columns alone); w_q is the corner's bilinear weight exactly as mdcn_backward forms it:
 * (1-ly)(1-lx), (1-ly)lx, ly(1-lx), ly lx for the fractional parts ly, lx of the sampling position.
 *     grad_input[n, y, x, c] = (sum over the element's terms of  rne(t / q_n))  * q_n
 * rne = round to nearest, ties to even, to an integer; the sum is exact (int64); the product with q_n is one rounding to
 * the arithmetic type.  The quantum is one per image: q_n = 2^e, the smallest power of two with
 *     A_n * G_n * bound <= 2^62 * q_n   (refined by up to three halvings while that still holds),
 * A_n = the largest finite |mask| of image n (1 without a mask), G_n = the largest finite |grad_columns| of image n,
 * bound = Ho*Wo*Kh*Kw: a tap's four corners are four different pixels, so an element receives at most one term per
 * (output pixel, tap), and bilinear weights are at most 1 -- no sum overflows.
 * Precision.  After the halvings A_n * G_n * bound > 2^61 * q_n, so q_n < A_n * G_n * bound * 2^-61: a term is off by at
 * most q_n / 2 < A_n * G_n * bound * 2^-62, and an element by at most (the terms it receives) * q_n / 2
 * <= A_n * G_n * bound^2 * 2^-62, before its one rounding to the arithmetic type.  The quantum grows with the map: at
 * 90x160 outputs and a 3x3 kernel (bound < 2^17) that is q_n / 2 < A_n * G_n * 2^-45 per term and A_n * G_n * 2^-28 per
 * element at the very most.  For fp32 arithmetic a term of magnitude A_n * G_n carries an ulp of 2^-24 of it, so the
 * quantisation is below the rounding the float-atomic sum makes at every add.  For MDCN_F64 it is not: a double's ulp is
 * 2^-53 of its magnitude, and q_n / 2 is coarser than that once bound exceeds about 2^9 (an 8x8 map with a 3x3 kernel) --
 * on larger maps the fixed-point fp64 result is reproducible but LESS precise than the fp64 float-atomic sum (still about
 * 2^-28 of A_n * G_n or better at the sizes above).
 * A non-finite term adds nothing to the sum; the element becomes what IEEE summation gives (NaN with a NaN term or with
 * infinities of both signs, else the infinity) and no other element is touched.
 * So the bits of grad_input[n] depend on image n's own tensors only: not on the run, the launch geometry, the batch the
 * image sits in, or how the caller cuts the batch into calls. */

/* Bytes of the workspace of mdcn_backward_input_fixed for `batch` images: the int64 accumulators [batch, H, W, C], one
 * class nibble per element (packed eight to a 32-bit word) and two 64-bit maxima per image, each of the three rounded up
 * to a multiple of 256 bytes; negative on a bad argument.  (shape->N is ignored.)  Host arithmetic only. */
long long mdcn_fixed_workspace_bytes(int dtype, const mdcn_shape *shape, int batch);

/* grad_input of mdcn_im2col as defined above, in three enqueued passes (maxima, scatter, conversion).
 *   grad_columns   [N*Ho*Wo, Kh*Kw*C], storage type; offset, mask (NULL: no modulation) as for mdcn_im2col;
 *   workspace      at least mdcn_fixed_workspace_bytes(dtype, shape, shape->N) bytes, 256-byte aligned, uninitialised:
 *                  the library zeroes what it needs;
 *   grad_input     [N, H, W, C] in the ARITHMETIC type (float; double for MDCN_F64), fully written.
 * There is no `input` pointer: grad_input does not depend on the input's values.  N == 0 is a no-op. */
int mdcn_backward_input_fixed(int dtype, const void *offset, const void *mask, const void *grad_columns,
                              const mdcn_shape *shape, void *workspace, void *grad_input, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MDCN_H */
