// What the fragment-stream convolutions share: K5 v5 (conv.hip: conv_frag_kernel), K14 (convblock.hip), K17 (convgru.hip) and K19 (convtail.hip)
// keep their pixel tiles in LDS and stream their weights as MFMA fragments from global memory through an 8-deep untracked register ring with
// counted waits (common.h: global_load16_async).  Here: the loader geometry of a tile, the ring's protocol -- start, K loop step, drain -- and
// the 1x1 layer on a resident tile of K14 and K19.
// The generated code depends on register allocation around the untracked loads: a kernel that cannot take a helper without its code object
// changing keeps the same text inline, with a comment that points here (tools/compare_code_objects.py is the judge).
#pragma once
#include "common.h"

namespace s2m2 {

// A tile of NPIX pixels x CH fp16 channels in LDS, loaded by NT threads in 16-byte pieces: thread t moves piece t % PPX of pixels
// t / PPX + RPI * it, it < A_IT.  Rows are padded by 16 bytes, and the tile has AROWS >= NPIX rows: every loader thread stashes all of its
// pieces, no exec-masked tail (conv.hip, load_halo, says what a masked tail would cost).
template <int NT, int CH, int NPIX>
struct HaloGeom {
    static constexpr int RS = CH + 8;                    // LDS row stride (elements)
    static constexpr int PPX = CH / 8;                   // 16-byte pieces per pixel
    static constexpr int RPI = NT / PPX;                 // pixels covered by one pass of the loader threads
    static constexpr int A_IT = (NPIX + RPI - 1) / RPI;  // passes
    static constexpr int AROWS = A_IT * RPI;
    static constexpr size_t A_BYTES = (size_t)AROWS * RS * 2;
    static_assert(NT % PPX == 0, "loader geometry");
};

// Starts a wave's stream at wf: fragments 0 .. KS-2 into slots 0 .. KS-2 ONLY.  Slot KS-1 gets its first request from step 0 of cb_steps.  A
// request made here for it would be one whose value is never consumed (step 0 overwrites it), and a destination whose value is never used is
// free for the allocator while the load is in flight (the hazard common.h describes): in K14 the allocator reused those registers under the
// load, a memory fault.  The stream has at least KS fragments.
template <int KS>
__device__ __forceinline__ void ring_start(raw16_t (&ring)[KS], const raw16_t* wf) {
#pragma unroll
    for (int s = 0; s < KS - 1; ++s) global_load16_async(ring[s], wf + (size_t)s * 64);
}

// Ends a stream: behind the last step the ring holds KS-1 re-requests of the stream's last fragment (cb_steps clamps).  They land, and every
// slot is consumed, before the registers are anything else's.
template <int KS>
__device__ __forceinline__ void ring_drain(raw16_t (&ring)[KS]) {
    wait_vmcnt<0>();
#pragma unroll
    for (int s = 0; s < KS; ++s) settle(ring[s]);
}

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
        // fragment g (slot kk) was requested KS - 1 steps ago; the KS - 2 requests made since then may still be in flight
        wait_vmcnt<KS - 2>();
        settle(ring[kk]);
        Frag<half_t> wfr;
        wfr.v = __builtin_bit_cast(half8_t, ring[kk]);
#pragma unroll
        for (int i = 0; i < MT; ++i) mma32(acc[i], wfr, xf[kk & 1][i]);   // D[cout][pixel]
        // refill the slot consumed one step ago (its MFMAs have long read their operands) with fragment g + KS - 1.
        // UNCONDITIONAL: a branch around an untracked load makes the compiler merge the two register states with copies
        // that read the slot while its load is in flight.  (So the stream's step 0 requests fragment KS - 1 into slot KS - 1: its first
        // request behind ring_start; behind v5's own fill of all KS slots, a re-request into its own slot.)
        {
            const int f = g + KS - 1;
            global_load16_async(ring[(kk + KS - 1) % KS], wf + (size_t)(f < nfrag ? f : nfrag - 1) * 64);
        }
        ++g;
    }
}

// A 1x1 layer (C -> 32 couts of this wave) on a tile resident in LDS: pixel tile i = rows 32 i + l31 of `tile` (TRS elements apart) against the
// wave's K9 fragments at wf, KS at a time as ordinary tracked loads (no ring: the caller's ring is drained, or not started yet)
template <int MT, int KS, int C, int TRS>
__device__ __forceinline__ void tile_1x1(float16_t (&acc)[MT], const half_t* tile, const raw16_t* wf, int l31, int hi) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll 1
    for (int c8 = 0; c8 < C / 16; c8 += KS) {
        raw16_t wr[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) wr[s] = global_load16(wf + (size_t)(c8 + s) * 64);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            Frag<half_t> wfr;
            wfr.v = __builtin_bit_cast(half8_t, wr[s]);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                Frag<half_t> xf;
                load_frag(xf, tile + (size_t)(32 * i + l31) * TRS + hi * 8 + (c8 + s) * 16);
                mma32(acc[i], wfr, xf);
            }
        }
    }
}

}  // namespace s2m2
