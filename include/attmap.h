/*
 * attmap.h -- C ABI of the mask head's multi-scale attention maps (DeVIS MultiScaleMHAttentionMap, one pyramid level per
 * call) in libmsda_hip.so: the masked softmax over all heads and pixels of q . k, fused so that the logits never exist in
 * memory.
 *
 * Geometry: B images, Q queries, n heads, c channels per head, an H x W map (P = H*W pixels).
 *
 *   logit[b,q,h,y,x] = scale * sum_c q[b,q,h,c] * k[b,h,c,y,x]        (-inf where mask[b,y,x] != 0)
 *   m[b,q]           = max of logit[b,q] over (h,y,x)
 *   s[b,q]           = sum of exp(logit[b,q] - m[b,q]) over (h,y,x)
 *   out[b,q,h,y,x]   = exp(logit - m[b,q]) / s[b,q]
 *
 * A masked pixel is exactly 0.  A row (b,q) whose pixels are all masked is NaN, as in the PyTorch formulation
 * (softmax of a row of -inf); no other row is affected.
 *
 * Backward.  With r[b,q] = sum over the row of grad_out * out and dL = out * (grad_out - r):
 *   grad_q[b,q,h,c]   = scale * sum_{y,x} dL[b,q,h,y,x] * k[b,h,c,y,x]
 *   grad_k[b,h,c,y,x] = scale * sum_q     dL[b,q,h,y,x] * q[b,q,h,c]
 * The library computes the softmax-gradient pass; the two contractions are the caller's batched GEMMs over the dl
 * buffer it writes, as the convolution's products with its weights are (mdcn.h):
 *   dl[b,h,q,p] = scale * dL[b,q,h,p]                                  ([B, n, Q, P]: a GEMM operand per (b,h) as it stands)
 *   grad_q[b,:,h,:] = dl[b,h] @ k[b,h]^T   ([Q,P] x [P,c])     grad_k[b,h] = q[b,:,h,:]^T @ dl[b,h]   ([c,Q] x [Q,P])
 * There are no float atomics anywhere: every sum of the library has a fixed order, so out and dl are bitwise reproducible
 * from run to run.
 *
 * Conventions (those of mdcn.h)
 *   - every pointer is a DEVICE pointer unless stated; tensors are dense:
 *       q [B, Q, n*c];  k [B, n*c, H, W] (NCHW as a 1x1 projection leaves it: pixels contiguous per channel);
 *       mask [B, H, W] bytes (non-zero = masked) or NULL;  out, grad_out [B, Q, n, H, W];
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work, never allocate and never
 *     synchronise (HIP-graph capture works), and are re-entrant;
 *   - `dtype` is an attmap_dtype: the storage type of q, k and dl.  `out_dtype` is the storage type of out and grad_out:
 *     `dtype` itself, or ATTMAP_F32 beside a 16-bit `dtype` -- nothing else.  Arithmetic is fp32, fp64 for ATTMAP_F64;
 *   - element offsets are 64-bit; B, n <= 65535, c <= 512, H*W < 2^31;
 *   - return value: ATTMAP_OK (0) or a negative attmap_status; on failure attmap_last_error() returns a thread-local
 *     message.  Arguments are checked before any HIP call, so argument errors are reported without a GPU.
 */
#ifndef ATTMAP_H
#define ATTMAP_H

#ifdef __cplusplus
extern "C" {
#endif

#define ATTMAP_ABI_VERSION 1

typedef enum attmap_status { ATTMAP_OK = 0, ATTMAP_ERR_ARGUMENT = -1, ATTMAP_ERR_HIP = -2 } attmap_status;

typedef enum attmap_dtype { ATTMAP_F32 = 0, ATTMAP_F64 = 1, ATTMAP_BF16 = 2, ATTMAP_F16 = 3 } attmap_dtype;

/* which gradients the caller will form from dl (attmap_backward) */
#define ATTMAP_GRAD_Q 1
#define ATTMAP_GRAD_K 2

typedef struct attmap_shape {
    int B, Q, n, c, H, W;
} attmap_shape;

int attmap_version(void);
const char *attmap_last_error(void);

/* Bytes of the workspace of attmap_forward and of attmap_backward (the larger of the two): per row (b,q), head and pixel
 * tile two values of the arithmetic type, rounded up to a multiple of 256 bytes; negative on a bad argument.  Host
 * arithmetic only. */
long long attmap_workspace_bytes(int dtype, const attmap_shape *shape);

/* out = the attention maps of q and k, in two enqueued passes:
 *   pass 1  per (row, head, pixel tile) the tile's maximum logit and its sum of exp(logit - maximum) -> workspace;
 *   pass 2  combines a row's partials in a fixed order, recomputes the logits and writes out.
 * out is written exactly once, every element, and never read.  workspace: at least attmap_workspace_bytes() bytes,
 * 16-byte aligned, uninitialised.  A row does not have to fit in on-chip memory.  B == 0 or Q == 0 is a no-op. */
int attmap_forward(int dtype, int out_dtype, const void *q, const void *k, const unsigned char *mask,
                   const attmap_shape *shape, double scale, void *workspace, void *out, void *stream);

/* The softmax-gradient pass for the gradients in `grads` (a mask of ATTMAP_GRAD_*; 0 is a no-op), in two enqueued passes:
 *   pass 1  per (row, head, pixel tile) the sum of grad_out * out -> workspace;
 *   pass 2  combines a row's partials in a fixed order into r[b,q] and writes dl[b,h,q,p] = scale * out * (grad_out - r).
 * dl [B, n, Q, H*W] in `dtype`'s storage type is written exactly once, every element.  Both gradients are contractions
 * of the same dl: `grads` does not change what is written.  workspace as for attmap_forward. */
int attmap_backward(int grads, int dtype, int out_dtype, const void *out, const void *grad_out, const attmap_shape *shape,
                    double scale, void *workspace, void *dl, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ATTMAP_H */
