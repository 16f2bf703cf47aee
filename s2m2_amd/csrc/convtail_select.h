// K19 patch selection as a pure function: which pixel patch s2m2_conv_block_tail gives a block.  Plain C++17 without HIP, like conv_select.h: a
// host-only program can tabulate it (tests/test_convtail_cpu.py holds it against conv_select_frag's choice for the same layer with S2M2_EPI_ADD).
#pragma once

namespace s2m2 {

struct ConvTailPatch {
    int ph, pw;
};

// The round-counting rule of conv_select_frag for a one-operand layer with its default tuning: v5 runs C / 128 blocks of 128 couts per patch on
// 512 block slots, K19 one block of C couts per patch on 512 * 128 / C slots -- the same number of rounds, so both are counted in v5's units.
// 4x40 patches where they save a round of blocks (5 MFMA tiles per block against 4, and never on grids of at most 256 blocks), else 2x32.
// force_ph x force_pw: 2x32, 4x32 or 4x40 force that patch (A/B and tests), anything else leaves the rule alone.
inline ConvTailPatch conv_tail_patch(int N, int H, int W, int C, int force_ph = 0, int force_pw = 0) {
    if ((force_ph == 2 && force_pw == 32) || (force_ph == 4 && (force_pw == 32 || force_pw == 40))) return {force_ph, force_pw};
    const long long slots = 512, small = 256, per_patch = C / 128;
    const long long b4 = (long long)N * ((W + 31) / 32) * ((H + 3) / 4) * per_patch;
    const long long b5 = (long long)N * ((W + 39) / 40) * ((H + 3) / 4) * per_patch;
    const long long cost4 = ((b4 + slots - 1) / slots) * 4, cost5 = ((b5 + slots - 1) / slots) * 5;
    if (b4 > small && cost5 < cost4 + 4) return {4, 40};
    return {2, 32};
}

}  // namespace s2m2
