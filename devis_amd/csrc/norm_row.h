// norm_row.h -- the row of the wave-per-row LayerNorm kernels, shared by prenorm.hip (include/prenorm.h) and swinends.hip
// (include/swinends.h): four consecutive elements of a lane, the channels a lane owns and the sums over a row in the order
// prenorm.h states -- g, then j, ascending in a lane, then butterflies.  Both units get the same bits from it.  Part of
// op_common.h, which includes it at its end (fp contraction is off there).
#ifndef NORM_ROW_H_
#define NORM_ROW_H_

namespace devis {
namespace normrow {

constexpr int kSpan = 256;                  // channels one group of four per lane covers: a row is G = ceil(C / kSpan) groups

// ---- four consecutive elements --------------------------------------------------------------------------------------------
template <typename T> struct alignas(sizeof(T) * 4 > 16 ? 16 : sizeof(T) * 4) Quad {
    T v[4];
};

// p[0..3] -> out, elements at or beyond `n` as 0; one 8 / 16-byte access when `vec` (nothing is dereferenced when n <= 0)
template <typename T> __device__ __forceinline__ void load4(const T *p, int n, bool vec, float (&out)[4])
{
    if (vec) {
        if (n > 0) {
            const Quad<T> q = *reinterpret_cast<const Quad<T> *>(p);
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = to_acc(q.v[j]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = 0.0f;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = j < n ? to_acc(p[j]) : 0.0f;
    }
}

template <typename T> __device__ __forceinline__ void store4(T *p, int n, bool vec, const float (&in)[4])
{
    if (vec) {
        if (n > 0) {
            Quad<T> q;
#pragma unroll
            for (int j = 0; j < 4; ++j) from_acc(q.v[j], in[j]);
            *reinterpret_cast<Quad<T> *>(p) = q;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) from_acc(p[j], in[j]);
    }
}

// v rounded to T, as the arithmetic type
template <typename T> __device__ __forceinline__ float rounded(float v)
{
    T t;
    from_acc(t, v);
    return to_acc(t);
}

// the first channel of group g of this lane
__device__ __forceinline__ int channel_of(int g, int lane) { return (g * 64 + lane) * 4; }

// the sum over the row's channels < C of v, in every lane: g, then j, ascending, then butterflies
template <int G> __device__ __forceinline__ float row_sum(const float (&v)[G][4], int C, int lane)
{
    float s = 0.0f;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) s += channel_of(g, lane) + j < C ? v[g][j] : 0.0f;
    return wave_sum(s);
}

// the same of the products a * b, each rounded on its own
template <int G> __device__ __forceinline__ float row_dot(const float (&a)[G][4], const float (&b)[G][4], int C, int lane)
{
    float s = 0.0f;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float t = a[g][j] * b[g][j];
            s += channel_of(g, lane) + j < C ? t : 0.0f;
        }
    return wave_sum(s);
}

// ---- host -------------------------------------------------------------------------------------------------------------------
template <int N> struct Groups { static constexpr int value = N; };

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }       // (NULL is aligned)

}  // namespace normrow
}  // namespace devis
#endif  // NORM_ROW_H_
