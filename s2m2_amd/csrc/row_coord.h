// Row -> (n, y, x) of an (N, Ho, Wo) pixel grid in 32-bit unsigned arithmetic: plain C++, host and device (no HIP header needed).
//
// The row-tile kernels (K10's z0 | z1 load, K9's pooled load, the pixel-shuffle stores of K11 / K5) give every thread a handful of
// 16-byte pieces whose rows are a compile-time distance apart.  Written per piece as m % Wo, m / Wo, t % Ho, t / Ho on 64-bit rows the
// decomposition costs two run-time divisions with a 64-bit slow path each, times the pieces of a thread.  Here a thread divides ONCE,
// for its first piece (32-bit: every entry point requires rows < 2^31), and walks on with adds and two carries:
//     K rows = dn images + dy image rows + dx columns   (block-uniform: one scalar division pair per kernel, none per piece)
//     x += dx, carry into y;  y += dy + carry, carry into n;  n += dn + carry
// x < Wo and dx < Wo, so x + dx < 2 Wo: one conditional subtraction settles it -- likewise y -- whatever the ratio of K to Wo
// (Wo = 1 included: dx = 0, dy = K % Ho, dn = K / Ho).  A walk may run past the last row of the tensor (the ragged last tile): n then
// counts images that do not exist, nothing overflows (m < 2^31 + a tile), and the caller masks those rows as it did before.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define S2M2_ROW_HD __host__ __device__ __forceinline__
#else
#define S2M2_ROW_HD inline
#endif

namespace s2m2 {

struct RowCoord {
    unsigned n, y, x;
};

// the walk over rows m, m + K, m + 2K, ... of an (N, Ho, Wo) grid; Ho, Wo >= 1
template <unsigned K>
struct RowWalk {
    unsigned Ho, Wo, dn, dy, dx;
    S2M2_ROW_HD RowWalk(unsigned Ho_, unsigned Wo_) : Ho(Ho_), Wo(Wo_) {
        const unsigned t = K / Wo_;
        dx = K - t * Wo_;
        dn = t / Ho_;
        dy = t - dn * Ho_;
    }
    S2M2_ROW_HD RowCoord decompose(unsigned m) const {
        const unsigned t = m / Wo, n = t / Ho;
        return RowCoord{n, t - n * Ho, m - t * Wo};
    }
    S2M2_ROW_HD void step(RowCoord& c) const {
        c.x += dx;
        const unsigned cx = c.x >= Wo;
        c.x -= cx ? Wo : 0u;
        c.y += dy + cx;
        const unsigned cy = c.y >= Ho;
        c.y -= cy ? Ho : 0u;
        c.n += dn + cy;
    }
};

// whether offsets inside ONE image of `pixels` rows of `stride` elements fit 32 bits (what the kernels' per-image offsets assume)
inline bool image_extent_fits_u32(long long pixels, long long stride) {
    return pixels > 0 && stride > 0 && pixels <= 0xffffffffLL / stride;
}

}  // namespace s2m2
