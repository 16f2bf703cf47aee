// The K loop step shared by the kernels that keep their pixel tiles in LDS and stream their weights as MFMA fragments from global memory
// through the 8-deep untracked register ring of K5 v5 (conv_frag_kernel): K14 (convblock.hip) and K18 (convgru.hip).
#pragma once
#include "common.h"

namespace s2m2 {

// KS k16 steps of one tap / one chunk of a 1x1 layer: MT pixel tiles from LDS (pixel fragments double buffered) against the ring's fragments.
// `g` = index of the fragment consumed next in this wave's stream of `nfrag` fragments at wf (16-byte units, stride 64 between fragments).
template <int MT, int KS>
__device__ __forceinline__ void cb_steps(float16_t (&acc)[MT], const half_t* a, const int (&poff)[MT], raw16_t (&ring)[KS], const raw16_t* wf,
                                         int& g, int nfrag) {
    Frag<half_t> xf[2][MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) load_frag(xf[0][i], a + poff[i]);
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
        if (kk + 1 < KS) {
#pragma unroll
            for (int i = 0; i < MT; ++i) load_frag(xf[(kk + 1) & 1][i], a + poff[i] + (kk + 1) * 16);
        }
        wait_vmcnt<KS - 2>();
        settle(ring[kk]);
        Frag<half_t> wfr;
        wfr.v = __builtin_bit_cast(half8_t, ring[kk]);
#pragma unroll
        for (int i = 0; i < MT; ++i) mma32(acc[i], wfr, xf[kk & 1][i]);
        {
            const int f = g + KS - 1;
            global_load16_async(ring[(kk + KS - 1) % KS], wf + (size_t)(f < nfrag ? f : nfrag - 1) * 64);
        }
        ++g;
    }
}

}  // namespace s2m2
