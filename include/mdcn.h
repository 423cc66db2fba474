/*
 * mdcn.h -- C ABI of the modulated deformable 2-D convolution (DCNv2; DCNv1 without a mask) in libmsda_hip.so:
 * the native operator of DeVIS's mask head (ModulatedDeformableConv2d, whose forward is one deform_conv2d call).
 *
 * The library holds the two kernels that are not a GEMM; the caller multiplies by the weights:
 *
 *   forward    mdcn_im2col   input, offset, mask -> columns [pixels, K*C]          out          = columns @ weight^T (+ bias)
 *   backward   (caller)      grad_columns [pixels, K*C] = grad_out @ weight        grad_weight  = grad_out^T @ columns
 *              mdcn_backward grad_columns, input, offset, mask -> grad_offset, grad_mask, and grad_input (accumulated)
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

#define MDCN_ABI_VERSION 1

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

#ifdef __cplusplus
}
#endif

#endif /* MDCN_H */
