// mask_taps.h -- the resampling rule of include/maskloss.h as the clip-stitching units evaluate it (maskiou.hip: the soft IoU
// operands and the binarised masks; maskrle.hip: the bits of the run-length encoder): per axis, in the arithmetic type, with
// the zero-weight-tap clause of include/maskiou.h.  One definition, so that the bits of maskrle_encode are those of
// maskiou_binarize by construction.
#ifndef MASK_TAPS_H_
#define MASK_TAPS_H_
#include "op_common.h"       // (fp contraction off)

namespace devis {

template <typename A> struct Tap {
    int i0, i1;
    A l0, l1;
};

// `scale` is (A)in / (A)out, formed once per thread
template <typename A> __device__ __forceinline__ Tap<A> tap_at(int d, int in, A scale)
{
    A r = scale * ((A)d + (A)0.5) - (A)0.5;
    r = r > (A)0 ? r : (A)0;
    Tap<A> t;
    t.i0 = (int)r;
    if (t.i0 > in - 1) t.i0 = in - 1;       // (never taken for a finite rule; keeps every index inside the map)
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = r - (A)t.i0;
    t.l0 = (A)1 - t.l1;
    return t;
}

// the resampled logit of one destination pixel from its four source values; a tap of weight 0 contributes nothing
// (include/maskiou.h)
template <typename A> __device__ __forceinline__ A lerp_of(const Tap<A> &ty, const Tap<A> &tx, A v00, A v01, A v10, A v11)
{
    const A top = tx.l0 * v00 + (tx.l1 == (A)0 ? (A)0 : tx.l1 * v01);
    const A bot = tx.l0 * v10 + (tx.l1 == (A)0 ? (A)0 : tx.l1 * v11);
    return ty.l0 * top + (ty.l1 == (A)0 ? (A)0 : ty.l1 * bot);
}

template <typename T> __device__ __forceinline__ typename Acc<T>::type logit_at(const T *__restrict__ sp, int w,
                                                                                const Tap<typename Acc<T>::type> &ty,
                                                                                const Tap<typename Acc<T>::type> &tx)
{
    typedef typename Acc<T>::type A;
    const T *ra = sp + (long long)ty.i0 * w, *rb = sp + (long long)ty.i1 * w;
    return lerp_of<A>(ty, tx, (A)to_acc(ra[tx.i0]), (A)to_acc(ra[tx.i1]), (A)to_acc(rb[tx.i0]), (A)to_acc(rb[tx.i1]));
}

}  // namespace devis
#endif  // MASK_TAPS_H_
