// K1 launch planning as a pure function: strips per image row, waves per block, chunks of right tokens and the cache policy of the volume stores
// of one s2m2_cost_volume launch.  Plain C++17 without HIP (tests/test_k1_cases_cpu.py tabulates it); ln_corr.hip launches what it returns and
// static_asserts that the block shapes restated here are the ones LnCorrCfg derives from its LDS and register budgets.
#pragma once

namespace s2m2 {

// Block shape of one (token bytes, cv bytes, C): most waves per block, the multiple they come in, right tokens a wave normalises per chunk.
// nwmax = 0: no such configuration.
struct LnCorrShape {
    int nwmax, nwgran, tpw;
};

constexpr LnCorrShape ln_corr_shape(int token_bytes, int cv_bytes, int C) {
    if (token_bytes == 2 && cv_bytes == 2)
        return C == 64 ? LnCorrShape{12, 1, 32} : C == 128 ? LnCorrShape{11, 1, 32} : C == 192 ? LnCorrShape{10, 2, 16}
             : C == 256 ? LnCorrShape{10, 2, 16} : C == 384 ? LnCorrShape{8, 2, 16} : LnCorrShape{0, 0, 0};
    if (token_bytes == 2 && cv_bytes == 4)                         // (the fp32 staging tile is twice as large: LDS cuts the wider blocks)
        return C == 64 ? LnCorrShape{12, 1, 32} : C == 128 ? LnCorrShape{9, 1, 32} : C == 192 ? LnCorrShape{10, 2, 16}
             : C == 256 ? LnCorrShape{8, 2, 16} : C == 384 ? LnCorrShape{6, 2, 16} : LnCorrShape{0, 0, 0};
    if (token_bytes == 4 && cv_bytes == 4)
        return C == 64 ? LnCorrShape{9, 1, 32} : C == 128 ? LnCorrShape{6, 1, 32} : C == 192 ? LnCorrShape{4, 1, 32}
             : C == 256 ? LnCorrShape{3, 1, 32} : C == 384 ? LnCorrShape{2, 1, 32} : LnCorrShape{0, 0, 0};
    return LnCorrShape{0, 0, 0};
}

struct LnCorrPlan {
    int nstrip;                     // blocks per image row: a block covers nw * 32 left pixels
    int nw;                         // waves per block
    int nchunks;                    // chunks of nw * tpw right tokens a block walks
    int store_mode;                 // store_cv's cache policy: 0 plain ... 4 (ln_corr.hip)
};

// store_env: S2M2_K1_NT (-1: not set)
inline LnCorrPlan ln_corr_plan(int B, int h, int w, int pitch, int token_bytes, int cv_bytes, int C, int store_env = -1) {
    const LnCorrShape s = ln_corr_shape(token_bytes, cv_bytes, C);
    LnCorrPlan p;
    const int tiles = (w + 31) / 32;                     // 32-pixel row tiles = waves needed per image row
    int nstrip = (tiles + s.nwmax - 1) / s.nwmax;
    // small problems: split rows into strips until the grid covers the chip (each strip re-reads / re-normalises the right row).  More, smaller
    // blocks do not help the 120-row case (c2): 240 three-wave blocks 12.1 us, 480-600 one- / two-wave blocks 14.6-15.6 us (profiles/r05/k1_minblocks.txt)
    while (B * h * nstrip < 200 && nstrip < tiles && (tiles + nstrip) / (nstrip + 1) >= 2) ++nstrip;
    int nw = (tiles + nstrip - 1) / nstrip;
    nw = (nw + s.nwgran - 1) / s.nwgran * s.nwgran;      // chunks of nw * TPW right tokens are whole 32-column tiles
    p.nstrip = nstrip;
    p.nw = nw;
    p.nchunks = (w + nw * s.tpw - 1) / (nw * s.tpw);
    // cache policy of the volume stores (store_cv): sc1 write-through by default -- measured (profiles/r04/k1_store_modes.txt, ab_k1_store_sc1lib_overlap.txt)
    // 19.2 -> 16.8 us back to back and 19.7-20.7 -> 17.7 us inside the forward against the write-back default of rounds 1-3; S2M2_K1_NT=0..4 A/B
    // (only for volume rows on 128-byte lines: a write-through store of a PARTIAL line is a read-modify-write at the memory side -- dense 608-byte
    // rows measured 25.0 us with sc1 against 21.8 with plain stores, profiles/r04/kbench.txt; the engine always allocates aligned rows)
    p.store_mode = store_env >= 0 ? store_env : ((pitch * cv_bytes) % 128 == 0 ? 2 : 0);
    return p;
}

}  // namespace s2m2
