// Host-side geometry and extent checks of the raster-order output stages K15 (cloud.hip), K18 (evalstats.hip) and K20 (mesh.hip): one definition
// of the extent bounds, the padded-map checks, the tile geometry and the workspace rounding.  Plain C++17 without HIP: a host-only program can
// call it (tools/operand_checks_host.cpp).
#pragma once
#include <stddef.h>

namespace s2m2 {

int set_error(const char* fmt, ...);            // common.h / runtime.hip: stores a thread-local message, returns 1

// B is a grid dimension (<= 65535); pixel indices of one pair and the per-pair counts are 32-bit (K20 passes 2^30: two faces per pixel)
inline bool raster_extents_ok(int B, int H, int W, long long max_pixels = 1LL << 31) {
    return B > 0 && H > 0 && W > 0 && (long long)H * W < max_pixels && B <= 65535;
}

// The (B, H, W) tensors against the padded (B, Hp, Wp) maps they are cropped from.  `entry` prefixes the message, `noun` names the unpadded
// tensor in it ("image", "ground truth").
inline int check_padded_maps(const char* entry, const char* noun, int B, int H, int W, int Hp, int Wp) {
    if (!(B > 0 && H > 0 && W > 0 && Hp > 0 && Wp > 0)) return set_error("%s: non-positive extents B=%d H=%d W=%d Hp=%d Wp=%d", entry, B, H, W, Hp, Wp);
    if (!(H <= Hp && W <= Wp)) return set_error("%s: the %s (H=%d, W=%d) is larger than the maps (Hp=%d, Wp=%d)", entry, noun, H, W, Hp, Wp);
    if (!(raster_extents_ok(B, H, W) && (long long)Hp * Wp < (1LL << 31))) return set_error("%s: extents too large (B <= 65535, H*W < 2^31)", entry);
    return 0;
}

// A tile: as many whole rows as fit into tile_pixels pixels (at least one); tiles of one pair; workspace sizes in whole 256-byte pieces
inline int tile_rows(int W, int tile_pixels) { return W >= tile_pixels ? 1 : tile_pixels / W; }
inline int tiles(int H, int rows) { return (int)(((long long)H + rows - 1) / rows); }      // (H = 2^31 - 1, W = 1 is a legal extent)
inline size_t round256(size_t n) { return (n + 255) / 256 * 256; }
// ... with more rows per tile where a pair would have more than max_tiles tiles (K18: its second launch loops over the tiles)
inline int tile_rows_capped(int H, int W, int tile_pixels, int max_tiles) {
    const int rows = tile_rows(W, tile_pixels);
    return tiles(H, rows) > max_tiles ? tiles(H, max_tiles) : rows;
}

}  // namespace s2m2
