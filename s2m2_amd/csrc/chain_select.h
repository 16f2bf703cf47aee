// K9 kernel selection as a pure function: form, tile height and block shape of the s2m2_mlp_chain launch for a validated descriptor.
// Plain C++17 without HIP (tests/test_select_cpu.py); chain.hip maps the choice to the instantiation.
#pragma once
#include "../../include/s2m2_hip.h"

namespace s2m2 {

struct ChainTuning {
    bool xcd_off = false;           // S2M2_K9_XCD=0           A/B: no XCD grouping of the row tiles
    int direct_bm = 0;              // S2M2_CHAIN_DIRECT_BM    tuning: 32 / 64 forces the direct form's tile height (C < 384)
};

enum class ChainForm { staged, direct, fan_only };     // weights staged in LDS / fragments straight from global memory / the same, fan-out layers only

struct ChainChoice {
    ChainForm form;
    int BM, NW, WP;                 // rows per tile, waves per block, weight tiles in flight through LDS (0: direct form)
    int xcd_tiles;                  // row tiles per XCD group (0: no grouping)
};

// C / dtype / nstage / nfan / weight_frag as mlp_chain_impl validated them.
inline ChainChoice chain_select(int C, int dtype, long long rows, int nstage, int nfan, int weight_frag, long long xcd_group_rows, const ChainTuning& t) {
    (void)nfan;                                                    // (every fan-out count runs on the kernel its stages choose)
    ChainChoice c;
    if (weight_frag) {
        // direct form: one wave per 32 couts; 32-row tiles while they fit the chip in about one round, else 64-row tiles (half the weight traffic
        // per row).  64-row tiles at 12 waves per block spill (55 - 88 registers); 16 waves: 128 registers each, 32-row tiles only
        const bool tall = C >= 384 ? false : t.direct_bm ? t.direct_bm == 64 : rows > (C == 128 ? 24576 : C == 192 ? 16384 : 8192);
        c.form = nstage == 0 ? ChainForm::fan_only : ChainForm::direct;
        c.BM = tall ? 64 : 32; c.NW = C / 32; c.WP = 0;
    } else {
        // staged form: at most one 32-row tile per CU -> short tiles, more CUs busy (measured: tools/chainbench.py)
        c.form = ChainForm::staged;
        c.BM = (dtype == S2M2_F32 || rows <= 8192 || C >= 384) ? 32 : 64;
        c.NW = (C == 128 || C == 384) ? 4 : 8; c.WP = 4;
    }
    const bool group = c.form != ChainForm::fan_only && xcd_group_rows > 0 && !t.xcd_off && xcd_group_rows % c.BM == 0 && rows % (8LL * xcd_group_rows) == 0;
    c.xcd_tiles = group ? (int)(xcd_group_rows / c.BM) : 0;
    return c;
}

}  // namespace s2m2
