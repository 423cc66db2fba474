// op_common.h -- what the translation units of the mask-path operators share (mdcn.hip / mdcn_det.hip, attmap.hip,
// mhstage.hip, maskloss.hip): the storage types, the float / double overloads of the kernels, the fixed-order wave and
// workgroup reductions, and the host side of an entry point -- sizes of the dtype codes, the error state behind
// <operator>_last_error() and the dispatch from a dtype code to a template instantiation.  The attention operator
// (msda_*.hip) has its own status codes and does not use this header.
#ifndef OP_COMMON_H_
#define OP_COMMON_H_
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdio.h>

#pragma clang fp contract(off)

namespace devis {

// The status and dtype codes of the four public headers, which each static_assert their own names against these.
enum { kOk = 0, kErrArgument = -1, kErrHip = -2 };
enum { kF32 = 0, kF64 = 1, kBF16 = 2, kF16 = 3 };

// ---- storage types: arithmetic in float, in double for double ------------------------------------------------
template <typename T> struct Acc { typedef float type; };
template <> struct Acc<double> { typedef double type; };

__device__ __forceinline__ float to_acc(float v) { return v; }
__device__ __forceinline__ double to_acc(double v) { return v; }
__device__ __forceinline__ float to_acc(__hip_bfloat16 v) { return __bfloat162float(v); }
__device__ __forceinline__ float to_acc(__half v) { return __half2float(v); }
__device__ __forceinline__ void from_acc(float &d, float v) { d = v; }
__device__ __forceinline__ void from_acc(double &d, double v) { d = v; }
__device__ __forceinline__ void from_acc(__hip_bfloat16 &d, float v) { d = __float2bfloat16(v); }
__device__ __forceinline__ void from_acc(__half &d, float v) { d = __float2half(v); }

// ---- one name for the float and the double function ----------------------------------------------------------
__device__ __forceinline__ float exp_of(float v) { return expf(v); }
__device__ __forceinline__ double exp_of(double v) { return exp(v); }
__device__ __forceinline__ float log1p_of(float v) { return log1pf(v); }
__device__ __forceinline__ double log1p_of(double v) { return log1p(v); }
__device__ __forceinline__ float pow_of(float a, float b) { return powf(a, b); }
__device__ __forceinline__ double pow_of(double a, double b) { return pow(a, b); }
__device__ __forceinline__ float fma_of(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double fma_of(double a, double b, double c) { return fma(a, b, c); }
__device__ __forceinline__ float max_of(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double max_of(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float rsqrt_of(float v) { return 1.0f / sqrtf(v); }
__device__ __forceinline__ double rsqrt_of(double v) { return 1.0 / sqrt(v); }
__device__ __forceinline__ float neg_inf(float) { return -INFINITY; }
__device__ __forceinline__ double neg_inf(double) { return -(double)INFINITY; }

// ---- reductions in a fixed order -----------------------------------------------------------------------------
// Butterflies over the 64 lanes: every lane ends with the same bits (max and IEEE add are commutative).  The order --
// xor 32, 16, ... 1, then the waves ascending -- is what makes the operators bitwise reproducible: it does not change.
template <typename A> __device__ __forceinline__ A wave_max(A v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max_of(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}
template <typename A> __device__ __forceinline__ A wave_sum(A v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the sum over a workgroup of WAVES waves in every thread: butterflies, then the waves in ascending order.  `red` holds
// WAVES values and is reusable after return.
template <int WAVES, typename A> __device__ __forceinline__ A block_sum(A v, A *red)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    A r = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r += red[w];
    __syncthreads();
    return r;
}

// ---- host ----------------------------------------------------------------------------------------------------
inline int elem_size(int dtype)     // 0 for a bad dtype code
{
    switch (dtype) {
    case kF32: return 4;
    case kF64: return 8;
    case kBF16: case kF16: return 2;
    default: return 0;
    }
}

inline int acc_size(int dtype) { return dtype == kF64 ? 8 : 4; }
inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

// The message behind <operator>_last_error().  Each operator has one thread_local instance of its own, so a failure
// of one never shows in another's message.
struct Status {
    char msg[512];

    void clear() { msg[0] = 0; }

    int fail(const char *fmt, long long a = 0, long long b = 0)
    {
        snprintf(msg, sizeof(msg), fmt, a, b);
        return kErrArgument;
    }

    int fail_hip(const char *what, hipError_t e)        // "<what>: <HIP's message>"
    {
        snprintf(msg, sizeof(msg), "%s: %s", what, hipGetErrorString(e));
        return kErrHip;
    }

    int check_launch(const char *what)
    {
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? kOk : fail_hip(what, e);
    }

    // the x dimension of a grid of `blocks` workgroups; `advice` ends the message of one that is too large
    int grid_of(long long blocks, unsigned *out, const char *advice = "")
    {
        if (blocks > 0x7fffffffLL) {
            snprintf(msg, sizeof(msg), "too many workgroups for one launch (%lld)%s", blocks, advice);
            return kErrArgument;
        }
        *out = (unsigned)blocks;
        return kOk;
    }
};

// From a (checked) dtype code to a template instantiation: f gets a Tag of the storage type, and in the two-type form
// a second one of the tensors that may be float32 beside a 16-bit dtype (`wide`).
//     dispatch(dtype, [&](auto t) { return launch<type_of<decltype(t)>>(...); })
template <typename T> struct Tag { typedef T type; };
template <typename G> using type_of = typename G::type;

template <typename F> int dispatch(int dtype, F &&f)
{
    switch (dtype) {
    case kF32: return f(Tag<float>());
    case kF64: return f(Tag<double>());
    case kBF16: return f(Tag<__hip_bfloat16>());
    default: return f(Tag<__half>());
    }
}

template <typename F> int dispatch(int dtype, bool wide, F &&f)
{
    switch (dtype) {
    case kF32: return f(Tag<float>(), Tag<float>());
    case kF64: return f(Tag<double>(), Tag<double>());
    case kBF16: return wide ? f(Tag<__hip_bfloat16>(), Tag<float>()) : f(Tag<__hip_bfloat16>(), Tag<__hip_bfloat16>());
    default: return wide ? f(Tag<__half>(), Tag<float>()) : f(Tag<__half>(), Tag<__half>());
    }
}

}  // namespace devis

#include "norm_row.h"        // devis::normrow: the row of the wave-per-row LayerNorm kernels (prenorm.hip, swinends.hip)
#endif  // OP_COMMON_H_
