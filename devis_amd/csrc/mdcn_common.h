// mdcn_common.h -- what the translation units of the modulated deformable convolution share (mdcn.hip: im2col and the
// default backward; mdcn_det.hip: the fixed-point grad_input): where a tap samples and its bilinear weights, and the host
// helpers of the entry points.  Both backward kernels take a tap's corners and weights from locate(), so they scatter the
// same products to the same elements.  The storage types and what every operator's host side needs are op_common.h.
#ifndef MDCN_COMMON_H_
#define MDCN_COMMON_H_
#include "op_common.h"
#include "mdcn.h"

namespace mdcn {

using namespace devis;

static_assert(MDCN_OK == kOk && MDCN_ERR_ARGUMENT == kErrArgument && MDCN_ERR_HIP == kErrHip, "status codes");
static_assert(MDCN_F32 == kF32 && MDCN_F64 == kF64 && MDCN_BF16 == kBF16 && MDCN_F16 == kF16, "dtype codes");

constexpr int kThreads = 256;       // 4 waves per workgroup

// ---- one tap of one output pixel -----------------------------------------------------------------------------
// Where tap k of output pixel `pix` (of this call's N*Ho*Wo) samples for offset group g, the four bilinear weights
// of the zero-extended input, and which corners exist.
template <typename A> struct Tap {
    long long row[4];   // element offset of corner (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1) in input [N, H, W, C]
    A w[4];             // bilinear weight of each corner
    A ly, lx;           // fractional parts
    bool ok[4];         // corner inside [0, H) x [0, W)
    bool inside;        // -1 < y < H and -1 < x < W: otherwise the tap samples zero and has zero gradients
    A m;                // mask value (1 without a mask)
    long long off_at;   // element offset of the row displacement in offset / grad_offset (the column one: + Ho*Wo)
    long long msk_at;   // element offset in mask / grad_mask
};

template <typename A, typename TO>
__device__ __forceinline__ Tap<A> locate(const mdcn_shape &s, const TO *__restrict__ off, const TO *__restrict__ msk,
                                         long long pix, int k, int g)
{
    Tap<A> t;
    const int K = s.Kh * s.Kw;
    const long long plane = (long long)s.Ho * s.Wo;
    const int wo = (int)(pix % s.Wo);
    const int ho = (int)((pix / s.Wo) % s.Ho);
    const long long n = pix / plane;
    const long long at = (long long)ho * s.Wo + wo;
    const int i = k / s.Kw, j = k - i * s.Kw;
    t.off_at = (n * (2 * s.G * K) + 2 * (g * K + k)) * plane + at;
    t.msk_at = (n * (s.G * K) + (g * K + k)) * plane + at;
    const A y = (A)(ho * s.stride_h - s.pad_h + i * s.dil_h) + (A)to_acc(off[t.off_at]);
    const A x = (A)(wo * s.stride_w - s.pad_w + j * s.dil_w) + (A)to_acc(off[t.off_at + plane]);
    t.m = msk ? (A)to_acc(msk[t.msk_at]) : (A)1;
    t.inside = y > (A)-1 && y < (A)s.H && x > (A)-1 && x < (A)s.W;       // (false for NaN)
    const A fy = t.inside ? floor(y) : (A)0, fx = t.inside ? floor(x) : (A)0;
    const int y0 = (int)fy, x0 = (int)fx;
    t.ly = t.inside ? y - fy : (A)0;
    t.lx = t.inside ? x - fx : (A)0;
    const A hy = (A)1 - t.ly, hx = (A)1 - t.lx;
    t.w[0] = hy * hx; t.w[1] = hy * t.lx; t.w[2] = t.ly * hx; t.w[3] = t.ly * t.lx;
    const bool y0in = t.inside && y0 >= 0, y1in = t.inside && y0 + 1 <= s.H - 1;
    const bool x0in = x0 >= 0, x1in = x0 + 1 <= s.W - 1;
    t.ok[0] = y0in && x0in; t.ok[1] = y0in && x1in; t.ok[2] = y1in && x0in; t.ok[3] = y1in && x1in;
    const long long base = ((n * s.H + y0) * s.W + x0) * s.C;
    t.row[0] = base; t.row[1] = base + s.C;
    t.row[2] = base + (long long)s.W * s.C; t.row[3] = t.row[2] + s.C;
    return t;
}

// ---- host (mdcn.hip) -----------------------------------------------------------------------------------------
extern thread_local Status err;     // mdcn_last_error(), of both translation units
int check_shape(const mdcn_shape *s);
int team_size(int Cg);      // lanes per (pixel, tap, group) of the backward kernels

// a dtype code as (code of input / columns, whether offset / mask are float32 beside them)
inline bool off32(int dtype) { return dtype == MDCN_BF16_OFF32 || dtype == MDCN_F16_OFF32; }
inline int input_code(int dtype) { return off32(dtype) ? dtype - MDCN_BF16_OFF32 + MDCN_BF16 : dtype; }
inline int check_dtype(int dtype) { return elem_size(input_code(dtype)) ? MDCN_OK : err.fail("bad dtype code %lld", dtype); }

// f(Tag<T>, Tag<TO>): T the type of input / columns, TO that of offset / mask
template <typename F> int dispatch_types(int dtype, F &&f) { return dispatch(input_code(dtype), off32(dtype), f); }

// the message of a grid that Status::grid_of refuses ends in this
constexpr const char *kFewerImages = ": call with fewer images";

}  // namespace mdcn
#endif  // MDCN_COMMON_H_
