// K29: edge-preserving smoothing of the disparity map (include/s2m2_hip.h: s2m2_smooth) -- a bilateral filter whose weights come from two
// tables formed on the host, so that no exponential is evaluated on the device and every byte of the result is defined.  One launch plus the
// clear of count:
//   smooth_kernel    a block owns a tile of kSmoothTileH rows x kSmoothTileW columns of the PADDED map of one pair (disp_out is the padded map:
//                    the same launch writes -1 to the border).  It evaluates K15's keep ONCE per pixel of the tile plus a halo of R rows and
//                    columns (cloud_device.h: cloud_eval4d, 16-byte map loads where the alignment allows) and leaves ONE plane in LDS: the
//                    map's disparity where the pixel is kept and inside the H x W crop, a NaN elsewhere -- a NaN fails the jump gate by
//                    itself, so a neighbour needs no second test.  A thread then owns four consecutive pixels of one row.  Per window row it
//                    takes the 4 + 2R disparities its four windows share out of LDS in 16-byte reads (1 + 2 * ceil(R / 4) of them) and walks
//                    the 2R + 1 taps of each pixel in registers; the radius is a template parameter so that this strip has constant indices
//                    (no scratch).  The range table lies in LDS next to the plane (S2M2_SMOOTH_WR_LDS = 0 reads it from the kernel
//                    arguments instead: profiles/smooth/smoothbench.txt has both); the spatial table is read from the kernel arguments at
//                    constant offsets, i.e. it lives in scalar registers.
// The tiles start at map column 0, so every group of four map pixels -- halo included -- is one aligned load that stays inside the padded row.
// The sum of a pixel is sequential in raster order of its window, as the rule demands: the four pixels of a thread are four independent chains.
#include "cloud_device.h"
#include "launch.h"
#include "plan.h"

#include <math.h>

#ifndef S2M2_SMOOTH_WR_LDS
#define S2M2_SMOOTH_WR_LDS 1
#endif

namespace s2m2 {

constexpr int kSmoothTileW = 64, kSmoothTileH = 16;      // 16 threads of four pixels x 16 rows = kRasterThreads
constexpr int kSmoothMaxRadius = 8;
constexpr int kSmoothRange = 256;                        // the range table has kSmoothRange + 1 entries
// LDS row stride in floats: 256 B = one bank row of the 16-byte reads.  A 16-lane group of ds_read_b128 takes lanes of two tile rows (lanes
// 0-3 and 12-15 of one, 4-11 of the next); with a stride of a whole bank row their 16 slots are the 16 distinct slots of one bank row, whatever
// the radius: no conflict.  (A stride of 64 + 8 * ceil(R / 4) floats would put the second row's slots on the first row's.)
constexpr int kSmoothLdsStride = 128;
static_assert(kSmoothTileW / 4 * kSmoothTileH == kRasterThreads, "one thread per group of four pixels");
static_assert(kSmoothTileW + 8 * ((kSmoothMaxRadius + 3) / 4) <= kSmoothLdsStride, "the halo fits the row");

struct SmoothParams {
    CloudParams c;              // the inputs of K15 (its outputs are null; rows_per_tile / tiles are not used)
    float* disp_out;            // (B,1,Hp,Wp)
    int* taps;                  // (B,1,H,W)
    int* count;
    int tiles_x;                // tiles across a padded row (blockIdx.x = tile row * tiles_x + tile column)
    float gate, inv;
    int vec_out, vec_taps;      // disp_out 16-byte aligned and Wp % 4 == 0; taps 16-byte aligned: a group may move whole
    float ws[kSmoothMaxRadius + 1];
    float wr[kSmoothRange + 1];
};

template <bool VEC, int R>
__global__ __launch_bounds__(kRasterThreads) void smooth_kernel(const SmoothParams p) {
#pragma clang fp contract(off)
    constexpr int HG = (R + 3) / 4;                          // halo groups on either side
    constexpr int LW = kSmoothTileW + 8 * HG, LH = kSmoothTileH + 2 * R;      // the filled part of the plane
    constexpr int NS = 4 + 8 * HG;                           // a thread's strip of one window row
    __shared__ int red[kRasterWaves];
    __shared__ __attribute__((aligned(16))) float ds[LH][kSmoothLdsStride];
#if S2M2_SMOOTH_WR_LDS
    __shared__ float wrl[kSmoothRange + 1];
#endif
    __shared__ float wsl[kSmoothMaxRadius + 1];
    const CloudParams& c = p.c;
    const int b = blockIdx.y;
    const int tile_y = (int)(blockIdx.x / (unsigned)p.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)p.tiles_x);
    const int v0 = tile_y * kSmoothTileH - c.oy, c0 = tile_x * kSmoothTileW - c.ox;       // the tile's first IMAGE row and column

    // the plane: LDS row 0 is image row v0 - R, LDS column 0 is image column c0 - 4 * HG
    for (int i = threadIdx.x; i < (LW / 4) * LH; i += kRasterThreads) {
        const int gy = i / (LW / 4), gx = i - gy * (LW / 4);
        const int v = v0 - R + gy, u0 = c0 - 4 * HG + 4 * gx;
        float z[4] = {0.f, 0.f, 0.f, 0.f}, d[4] = {0.f, 0.f, 0.f, 0.f};
        // a group with a pixel inside the crop: its map column ox + u0 is a multiple of four in [0, Wp)
        if (v >= 0 && v < c.H && u0 + 3 >= 0 && u0 < c.W) cloud_eval4d<VEC>(c, b, v, u0, z, d);
#pragma unroll
        for (int j = 0; j < 4; ++j) ds[gy][4 * gx + j] = z[j] > 0.f ? d[j] : __builtin_nanf("");
    }
#if S2M2_SMOOTH_WR_LDS
    for (int i = threadIdx.x; i <= kSmoothRange; i += kRasterThreads) wrl[i] = p.wr[i];
#endif
    if (threadIdx.x <= kSmoothMaxRadius) wsl[threadIdx.x] = p.ws[threadIdx.x];
    __syncthreads();

    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int v = v0 + ty, u0 = c0 + tx * 4;
    const int my = v + c.oy, mx = u0 + c.ox;                 // the group's map row and first map column (a multiple of four)
    int n_kept = 0;
    if (my < c.Hp && mx < c.Wp) {
        float out[4], dc[4];
        int taps[4] = {0, 0, 0, 0};
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dc[j] = ds[R + ty][4 * HG + 4 * tx + j];         // a NaN: not kept, or outside the crop
            out[j] = -1.f;
            any = any || dc[j] == dc[j];
        }
        if (any) {
            float num[4] = {0.f, 0.f, 0.f, 0.f}, den[4] = {0.f, 0.f, 0.f, 0.f};
            for (int dv = -R; dv <= R; ++dv) {
                float s[NS];
#pragma unroll
                for (int g = 0; g < NS / 4; ++g) {
                    const raw16_t q = *reinterpret_cast<const raw16_t*>(&ds[R + ty + dv][4 * tx + 4 * g]);
#pragma unroll
                    for (int k = 0; k < 4; ++k) s[4 * g + k] = q[k];
                }
                const float wv = wsl[dv < 0 ? -dv : dv];
#pragma unroll
                for (int du = -R; du <= R; ++du) {
                    const float wvu = wv * p.ws[du < 0 ? -du : du];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float e = s[4 * HG + j + du] - dc[j];
                        const float a = fabsf(e);
                        const float t = fminf(a * p.inv, (float)kSmoothRange);
                        const int i = (int)t;
#if S2M2_SMOOTH_WR_LDS
                        const float w = wvu * wrl[i];
#else
                        const float w = wvu * p.wr[i];
#endif
                        const float we = w * e;
                        if (a <= p.gate) {                   // a NaN fails: a neighbour that is not kept, a centre that is not kept
                            num[j] = num[j] + we;
                            den[j] = den[j] + w;
                            ++taps[j];
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (dc[j] == dc[j]) {
                    const float q = num[j] / den[j];
                    out[j] = dc[j] + q;
                    ++n_kept;
                } else {
                    taps[j] = 0;
                }
            }
        }
        if (p.disp_out) {
            const size_t m = ((size_t)b * c.Hp + my) * (size_t)c.Wp + (size_t)mx;
            if (p.vec_out) {
                const raw16_t o = {out[0], out[1], out[2], out[3]};
                *reinterpret_cast<raw16_t*>(p.disp_out + m) = o;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (mx + j < c.Wp) p.disp_out[m + j] = out[j];
            }
        }
        if (p.taps && v >= 0 && v < c.H && u0 + 3 >= 0 && u0 < c.W)
            dense_store4(p.taps, raster_dense_row(c, b, v), u0, c.W, p.vec_taps != 0, taps);
    }
    if (p.count) {
        n_kept = block_sum_int(n_kept, red);
        if (threadIdx.x == 0 && n_kept) atomicAdd(p.count + b, n_kept);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host

static int smooth_tables(const char* what, int radius, double sigma_s, double sigma_r, float* ws, float* wr, float* inv) {
    S2M2_REQUIRE(radius >= 1 && radius <= kSmoothMaxRadius, "%s: radius must be 1..%d (%d)", what, kSmoothMaxRadius, radius);
    S2M2_REQUIRE(isfinite(sigma_s) && sigma_s > 0.0, "%s: sigma_s must be finite and > 0 (%g)", what, sigma_s);
    S2M2_REQUIRE(isfinite(sigma_r) && sigma_r > 0.0, "%s: sigma_r must be finite and > 0 (%g)", what, sigma_r);
    for (int k = 0; k <= kSmoothMaxRadius; ++k) ws[k] = k <= radius ? (float)exp(-(double)(k * k) / (2.0 * sigma_s * sigma_s)) : 0.f;
    const double step = 4.0 * sigma_r / (double)kSmoothRange;
    for (int i = 0; i <= kSmoothRange; ++i) {
        const double e = (double)i * step;
        wr[i] = (float)exp(-(e * e) / (2.0 * sigma_r * sigma_r));
    }
    *inv = (float)((double)kSmoothRange / (4.0 * sigma_r));
    return 0;
}

template <bool VEC>
static int smooth_launch(int radius, dim3 grid, hipStream_t s, const SmoothParams& p) {
    const dim3 block(kRasterThreads);
    switch (radius) {
        case 1: return launch<smooth_kernel<VEC, 1>>("smooth", grid, block, 0, s, p);
        case 2: return launch<smooth_kernel<VEC, 2>>("smooth", grid, block, 0, s, p);
        case 3: return launch<smooth_kernel<VEC, 3>>("smooth", grid, block, 0, s, p);
        case 4: return launch<smooth_kernel<VEC, 4>>("smooth", grid, block, 0, s, p);
        case 5: return launch<smooth_kernel<VEC, 5>>("smooth", grid, block, 0, s, p);
        case 6: return launch<smooth_kernel<VEC, 6>>("smooth", grid, block, 0, s, p);
        case 7: return launch<smooth_kernel<VEC, 7>>("smooth", grid, block, 0, s, p);
        default: return launch<smooth_kernel<VEC, 8>>("smooth", grid, block, 0, s, p);
    }
}

static int smooth_impl(const s2m2_smooth_desc* d, void* stream) {
    S2M2_REQUIRE(d != nullptr, "smooth: null descriptor");
    if (int rc = refuse_while_recording("smooth")) return rc;
    SmoothParams p;
    bool vec = false;
    s2m2_cloud_desc in = d->cloud;                  // the inputs alone: the output fields of the embedded descriptor are ignored
    in.depth = nullptr; in.mask = nullptr; in.records = nullptr; in.count = nullptr; in.workspace = nullptr; in.capacity = 0;
    if (int rc = cloud_validate(&in, "smooth", kCloudTilePixels, p.c, vec, false)) return rc;
    S2M2_REQUIRE(d->disp_out || d->taps || d->count, "smooth: no output requested (disp_out, taps and count are all null pointers)");
    S2M2_REQUIRE((((uintptr_t)d->disp_out | (uintptr_t)d->taps | (uintptr_t)d->count) & 3) == 0,
                 "smooth: disp_out, taps and count must be 4-byte aligned");
    S2M2_REQUIRE(d->max_jump >= 0.0, "smooth: max_jump must be >= 0 (%g)", d->max_jump);                   // false for a NaN
    if (int rc = smooth_tables("smooth", d->radius, d->sigma_s, d->sigma_r, p.ws, p.wr, &p.inv)) return rc;
    if (d->disp_out) {                              // a block reads halo pixels that another block's tile covers: in place is a race
        const size_t bytes = (size_t)d->cloud.B * d->cloud.Hp * d->cloud.Wp * sizeof(float);
        const uintptr_t o0 = (uintptr_t)d->disp_out, o1 = o0 + bytes;
        const void* maps[3] = {d->cloud.disp, d->cloud.occ, d->cloud.conf};
        for (const void* m : maps) {
            const uintptr_t a0 = (uintptr_t)m, a1 = a0 + bytes;
            S2M2_REQUIRE(o1 <= a0 || a1 <= o0, "smooth: disp_out overlaps an input map");
        }
    }

    p.disp_out = d->disp_out; p.taps = d->taps; p.count = d->count;
    p.tiles_x = (int)(((long long)p.c.Wp + kSmoothTileW - 1) / kSmoothTileW);
    p.gate = (float)d->max_jump;
    p.vec_out = ((uintptr_t)d->disp_out & 15) == 0 && p.c.Wp % 4 == 0;
    p.vec_taps = ((uintptr_t)d->taps & 15) == 0;

    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d->count && hipMemsetAsync(d->count, 0, sizeof(int) * (size_t)d->cloud.B, s) != hipSuccess) return set_error("smooth: memset failed");
    const int tiles_y = (int)(((long long)p.c.Hp + kSmoothTileH - 1) / kSmoothTileH);
    const dim3 grid((unsigned)(p.tiles_x * tiles_y), d->cloud.B);                              // tiles_x * tiles_y <= Hp * Wp < 2^31
    return vec ? smooth_launch<true>(d->radius, grid, s, p) : smooth_launch<false>(d->radius, grid, s, p);
}

static int smooth_weights_impl(int radius, double sigma_s, double sigma_r, float* ws9, float* wr257, float* inv) {
    S2M2_REQUIRE(ws9 && wr257 && inv, "smooth_weights: null pointer (ws9 / wr257 / inv)");
    return smooth_tables("smooth_weights", radius, sigma_s, sigma_r, ws9, wr257, inv);
}

}  // namespace s2m2

extern "C" int s2m2_smooth(const s2m2_smooth_desc* desc, void* stream) { return s2m2::smooth_impl(desc, stream); }
extern "C" int s2m2_smooth_weights(int radius, double sigma_s, double sigma_r, float* ws9, float* wr257, float* inv) {
    return s2m2::smooth_weights_impl(radius, sigma_s, sigma_r, ws9, wr257, inv);
}
