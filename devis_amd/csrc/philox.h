// philox.h -- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) as the dropout masks of
// addnorm.hip and selfattn.hip draw it (include/addnorm.h, include/selfattn.h: key = the seed's two words, counter = what the
// operator's header says).  Integer arithmetic only: the words do not depend on the unit that includes this.
#ifndef PHILOX_H_
#define PHILOX_H_
#include <hip/hip_runtime.h>

namespace devis {

__device__ __forceinline__ void philox4x32_10(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                              unsigned (&out)[4])
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

}  // namespace devis
#endif  // PHILOX_H_
