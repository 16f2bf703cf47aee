// K5 kernel selection as a pure function: which kernel family and which instantiation s2m2_conv2d launches for a validated layer, a `tile` id
// and the tuning switches.  Plain C++17 without HIP: a host-only program can call it, tabulate it and diff it (tests/test_select_cpu.py).
// conv.hip maps the choice to the instantiation and launches it.
#pragma once
#include <stddef.h>
#include <stdio.h>

#include "../../include/s2m2_hip.h"

namespace s2m2 {

// The K5 environment switches, read once per process by conv.hip: conv_tuning().
struct ConvTuning {
    int frag_ph = 0;                // S2M2_FRAG_PH      A/B: 2 / 4 force the patch height of the K-order-2 kernel (128-cout blocks)
    int frag_pw = 0;                // S2M2_FRAG_PW      A/B: 40 forces 4x40 patches on plain layers, 32 switches them off (128-cout blocks)
    int frag_aux_pw = 40;           // S2M2_FRAG_AUX_PW  A/B: 32 = one-operand layers on 64-pixel blocks only (128-cout blocks)
    long long t20_min = 300;        // S2M2_T20_MIN      tuning: fewest 128x128 tiles for the 8-wave tile
    int small_tile = 0;             // S2M2_SMALL_TILE   tile id for what is left over (0: 6 / 2 by K)
    bool no_halo8 = false;          // S2M2_CONV_NO_HALO8  A/B, "set at all": no 8-wave halo tiles
    long long halo_big_min = 30000; // S2M2_HALO_BIG_MIN tuning: fewest pixels for tile 26
    int halo_narrow = 13;           // S2M2_HALO_NARROW  halo tile id below 128 couts
    int halo_coarse = 24;           // S2M2_HALO_COARSE  halo tile id for short grids
    bool npf = false;               // S2M2_CONV_NPF     A/B, "set at all": 4 K tiles in flight for the v1 tiles
};

enum class ConvFamily { error, igemm, igemm2, halo, frag, pw };

// The chosen family with its template parameters, in the order the launchers of conv.hip take them (defaults filled in):
//   igemm  BM, BN, WGM, PPR, NPF, NWAVES, MODE        igemm2  BM, BN, KP, NS        halo  BN, NWAVES, WGM, DW
//   frag   BN, CH, PH, PW, AUX (epilogue operands parked in registers)              pw    BN
// or family error with the formatted message.
struct ConvChoice {
    ConvFamily family = ConvFamily::error;
    int p[7] = {0, 0, 0, 0, 0, 0, 0};
    char error[200] = "";
    bool is(ConvFamily f, int p0, int p1 = 0, int p2 = 0, int p3 = 0, int p4 = 0, int p5 = 0, int p6 = 0) const {
        return family == f && p[0] == p0 && p[1] == p1 && p[2] == p2 && p[3] == p3 && p[4] == p4 && p[5] == p5 && p[6] == p6;
    }
};

namespace conv_select_detail {

inline ConvChoice pick(ConvFamily f, int p0, int p1 = 0, int p2 = 0, int p3 = 0, int p4 = 0, int p5 = 0, int p6 = 0) {
    ConvChoice c;
    c.family = f;
    const int p[7] = {p0, p1, p2, p3, p4, p5, p6};
    for (int i = 0; i < 7; ++i) c.p[i] = p[i];
    return c;
}
template <typename... V>
inline ConvChoice refuse(const char* fmt, V... v) {
    ConvChoice c;
    if constexpr (sizeof...(V) == 0) snprintf(c.error, sizeof(c.error), "%s", fmt);
    else snprintf(c.error, sizeof(c.error), fmt, v...);
    return c;
}
inline ConvChoice igemm(int BM, int BN, int WGM, int PPR = 8, int NPF = 1, int NWAVES = 4, int MODE = 0) {
    return pick(ConvFamily::igemm, BM, BN, WGM, PPR, NPF, NWAVES, MODE);
}
inline ConvChoice igemm2(int BM, int BN, int KP, int NS) { return pick(ConvFamily::igemm2, BM, BN, KP, NS); }

template <typename Args>
inline ConvChoice halo(const Args& a, int BN, int NWAVES = 4, int WGM = 2, int DW = 1) {
    if (a.stride != 1 || a.shuffle2 || a.korder || a.KH > 3 || a.KW > 3) return refuse("conv2d: the halo tile needs a stride-1 kernel of at most 3x3 taps in K order 0");
    return pick(ConvFamily::halo, BN, NWAVES, WGM, DW);
}

}  // namespace conv_select_detail

// LDS bytes of the persistent pointwise kernel (ConvCfgP: two 64-pixel activation buffers of 128-byte rows, the staging tile, the weight slice)
constexpr size_t conv_pw_lds_bytes(int BN, int K, size_t elem) {
    const size_t vec = 16 / elem;
    return ((size_t)2 * 64 * 9 * vec + (size_t)64 * (BN + vec) + (size_t)BN * (K + vec)) * elem;
}

template <typename Args>
inline ConvChoice conv_select_pw(const Args& a, bool fp16, int BN) {
    using namespace conv_select_detail;
    if (a.KH != 1 || a.KW != 1 || a.stride != 1) return refuse("conv2d: the pointwise kernel needs a 1x1 stride-1 layer");
    const size_t lds = conv_pw_lds_bytes(BN, a.Cin, fp16 ? 2 : 4);
    if (lds > 160 * 1024) return refuse("conv2d: pointwise kernel: Cin=%d needs %zu bytes of LDS", a.Cin, lds);
    return pick(ConvFamily::pw, BN);
}

// K order 2 (weights packed as a fragment stream, fp16): blocks of `cb` couts on 2x32, 4x32 or 4x40 pixel patches.  The cost model counts rounds
// of the `slots` co-resident block slots of the chip times the MFMA tiles per block (4 / 5); grids of at most `small` 128-pixel blocks take
// 64-pixel blocks, and so does every layer with an epilogue operand (4 operand pieces per thread instead of 8).  tile: 2 / 4 force the patch
// height, 40 the 4x40 patch.
template <typename Args>
inline ConvChoice conv_select_frag(const Args& a, int tile, int cb, int slots, int small, int force_ph, int force_pw, int aux_pw) {
    using namespace conv_select_detail;
    const long long b4 = (long long)a.N * ((a.W + 31) / 32) * ((a.H + 3) / 4) * (a.Cout / cb);
    const long long b5 = (long long)a.N * ((a.W + 39) / 40) * ((a.H + 3) / 4) * (a.Cout / cb);
    const long long cost4 = ((b4 + slots - 1) / slots) * 4, cost5 = ((b5 + slots - 1) / slots) * 5;
    const bool one_op = a.epi == S2M2_EPI_ADD || a.epi == S2M2_EPI_MUL;
    int ph, pw;
    if (tile == 2 || tile == 4 || tile == 40) {                   // a forced form is taken as it is or refused below, never replaced by another
        ph = tile == 2 ? 2 : 4;
        pw = tile == 40 ? 40 : 32;
    } else {
        const int PH = (force_ph == 2 || force_ph == 4) ? force_ph : (a.epi != S2M2_EPI_NONE || b4 <= small) ? 2 : 4;
        bool wide = false;
        if (one_op && tile == 0 && aux_pw == 40 && force_ph == 0) wide = b4 > small && cost5 < cost4 + 4;
        else if (PH == 4 && a.epi == S2M2_EPI_NONE) wide = force_pw == 40 || (tile == 0 && force_pw != 32 && cost5 < cost4);
        ph = wide ? 4 : PH;
        pw = wide ? 40 : 32;
    }
    // what the kernel can take
    const bool two = a.epi == S2M2_EPI_GRU || a.epi == S2M2_EPI_GATEMIX;
    const int naux = a.epi == S2M2_EPI_NONE ? 0 : two ? 2 : 1;
    if (a.stride != 1 || a.shuffle2 || a.KH > 3 || a.KW > 3 || a.KH * a.KW < 2 || a.Cout % cb || a.Cin % 8 || a.ln_wsum)
        return refuse("conv2d: K order 2 needs a stride-1 3x3 / 3x1 / 1x3 layer with Cout a multiple of %d (Cout=%d)", cb, a.Cout);
    if (pw != 32 && naux == 2) return refuse("conv2d: K order 2 with 160-pixel blocks takes one-operand epilogues only (epi=%d has two)", a.epi);
    if (a.epi == S2M2_EPI_DUALMIX || (ph == 4 && two))
        return refuse("conv2d: K order 2 with 128-pixel blocks takes one-operand epilogues only (epi=%d has two)", a.epi);
    return pick(ConvFamily::frag, cb, cb, ph, pw, naux);
}

// Args: the fields of conv.hip's ConvArgs that selection reads -- N, H, W, Ho, Wo, KH, KW, Cin, Cout, stride, epi, shuffle2, korder, pool2 and
// ln_wsum (tested for null / zero only) -- of a layer that conv2d_impl's validation accepted.  tile: 0 = the heuristic, otherwise the id to force.
template <typename Args>
inline ConvChoice conv_select(const Args& a, int tile, bool fp16, const ConvTuning& t) {
    using namespace conv_select_detail;
    const long long M = (long long)a.N * a.Ho * a.Wo;
    const bool auto_tile = tile == 0;
    if (a.korder == 2) {                                          // weights packed as a fragment stream: one kernel takes them
        if (!fp16) return refuse("conv2d: K order 2 (fragment stream) is an fp16 layout");
        // Cout a multiple of 192 but not of 128 with Cin a multiple of 192 (the M model's C = 192 layers): blocks of 192 couts (six waves) on
        // 192-channel chunks -- one block per CU (100 KB halo tile), 256 block slots per round; this path has no A/B switches.  Otherwise blocks
        // of 128 couts, two per CU: 512 slots
        if (s2m2_conv_frag_chunk(a.Cout, a.Cin) == 192) return conv_select_frag(a, tile, 192, 256, 128, 0, 0, 40);
        return conv_select_frag(a, tile, 128, 512, 256, t.frag_ph, t.frag_pw, t.frag_aux_pw);
    }
    if (a.pool2) {                                                // AvgPool2d(2) + 1x1 (the coarse grids): 64x64 tiles, 64- / 128-byte K rows
        if (tile == 2 || (tile != 6 && a.Cin > 512)) return igemm(64, 64, 2, 8, 1, 4, 3);
        return igemm(64, 64, 2, 4, 1, 4, 3);
    }
    if (tile == 0) {                                              // measured on MI355X (tools/convbench.py, profiles/r01)
        const int Ktot = a.KH * a.KW * a.Cin;
        if (a.KH * a.KW > 1 && a.KH <= 3 && a.KW <= 3 && a.stride == 1 && !a.shuffle2 && !a.korder && a.Cin > 16)
            // spatial kernels: halo tile; 8 waves x 128 couts when there is enough work (8-wave tiles with 2 / 4 weight tiles in flight)
            tile = (a.Cout >= 128 && !t.no_halo8) ? (M >= t.halo_big_min ? 26 : t.halo_coarse) : t.halo_narrow;
        else if (a.KH * a.KW > 1 && a.Cin <= 16 && a.stride == 1) tile = 6;   // spatial kernel on <= 16 channels: a 128-byte halo chunk would be
                                                                      // mostly padding; K = taps x channels packed densely instead (8->32 full res: 108 vs 156 us)
        else if (a.Cout <= 32) tile = 3;                               // 128x32: narrow heads
        else if (a.Cout >= 128 && ((M + 127) / 128) * ((a.Cout + 127) / 128) >= t.t20_min) tile = 20;  // 128x128, 64-byte K rows, 8 waves
        else tile = t.small_tile ? t.small_tile : (Ktot <= 512 ? 6 : 2);   // 64x64 with 64- / 128-byte K rows
        if (t.npf && !a.ln_wsum) tile = tile == 6 ? 16 : tile == 2 ? 17 : tile == 20 ? 27 : tile;
    }
    if (a.ln_wsum) {                                              // pre-LN folded in: the v1 tiles the heuristic picks for 1x1 layers
        switch (tile) {
            case 2: return igemm(64, 64, 2, 8, 1, 4, 1);
            case 3: return igemm(128, 32, 4, 8, 1, 4, 1);
            case 6: return igemm(64, 64, 2, 4, 1, 4, 1);
            case 20: return igemm(128, 128, 2, 4, 1, 8, 1);
            default: return refuse("conv2d: tile %d has no pre-LayerNorm variant (2, 3, 6, 20 do)", tile);
        }
    }
    if (a.epi == S2M2_EPI_DUALMIX) {                              // two GEMMs, one launch: the v1 tiles the heuristic picks for 1x1 layers
        if (auto_tile) tile = 2;                                  // measured end to end: 64x64 / 128-byte K rows (the 8-wave 128x128 tile needs 168 VGPRs with two accumulator sets: one block per CU)
        switch (tile) {
            case 2: return igemm(64, 64, 2, 8, 1, 4, 2);
            case 6: return igemm(64, 64, 2, 4, 1, 4, 2);
            case 20: return fp16 ? igemm(128, 128, 2, 4, 1, 8, 2) : igemm(64, 64, 2, 8, 1, 4, 2);   // fp32: 64x64 tiles only (4 staged pieces per thread)
            default: return refuse("conv2d: tile %d has no dual-GEMM variant (2, 6, 20 do)", tile);
        }
    }
    switch (tile) {
        case 1: return igemm(128, 128, 2);
        case 2: return igemm(64, 64, 2);
        case 3: return igemm(128, 32, 4);
        case 4: return igemm(128, 64, 2);
        case 5: return igemm(128, 128, 2, 4);                      // 64-byte K rows: half the LDS, 3 blocks per CU
        case 6: return igemm(64, 64, 2, 4);
        case 7: return igemm2(128, 128, 1, 4);                     // v2 (LDS-direct ring): 64 KB, 3 tiles ahead
        case 8: return igemm2(128, 128, 2, 2);                     // v2: 128-byte K rows, 1 tile ahead
        case 9: return igemm2(128, 128, 2, 3);                     // v2: 96 KB, 2 tiles ahead
        case 10: return igemm2(64, 64, 2, 4);                      // v2: 64x64, 64 KB
        case 11: return igemm2(64, 64, 1, 4);                      // v2: 64x64, 32 KB
        case 12: return halo(a, 128);                              // v3 halo tile, 4x32 pixel patch x 128 couts
        case 13: return halo(a, 64);                               // v3 halo tile, x 64 couts
        case 14: return conv_select_pw(a, fp16, 128);              // v4 persistent pointwise, 128 couts per block
        case 15: return conv_select_pw(a, fp16, 64);               // v4 persistent pointwise, 64 couts per block
        case 16: return igemm(64, 64, 2, 4, 4);                    // 64x64, 64-byte K rows, 4 K tiles in flight
        case 17: return igemm(64, 64, 2, 8, 4);                    // 64x64, 128-byte K rows, 4 K tiles in flight
        case 18: return igemm(128, 128, 2, 4, 4);                  // 128x128, 64-byte K rows, 4 K tiles in flight
        case 19: return halo(a, 128, 8);                           // v3 halo tile, 128 couts, 8 waves (32 couts per wave)
        case 20: return igemm(128, 128, 2, 4, 1, 8);               // 128x128, 64-byte K rows, 8 waves (64 px x 32 couts each)
        case 21: return igemm(128, 128, 2, 8, 1, 8);               // 128x128, 128-byte K rows, 8 waves
        case 22: return igemm(64, 128, 2, 4, 1, 8);                // 64x128, 64-byte K rows, 8 waves (32 px x 32 couts each)
        case 23: return halo(a, 64, 8, 4);                         // v3 halo tile, 64 couts, 8 waves (one patch row x 32 couts each)
        case 24: return halo(a, 64, 8, 4, 4);                      // t23 with 4 weight tiles in flight (short grids)
        case 25: return halo(a, 64, 4, 2, 4);                      // t13 with 4 weight tiles in flight
        case 26: return halo(a, 128, 8, 2, 2);                     // t19 with 2 weight tiles in flight
        case 27: return igemm(128, 128, 2, 4, 4, 8);               // t20 with 4 K tiles in flight
        default: return refuse("conv2d: unknown tile id %d", tile);
    }
}

}  // namespace s2m2
