// K28: the normal map of the disparity map (include/s2m2_hip.h: s2m2_normals) -- per kept pixel the cross product of the vertical and the
// horizontal difference of the back-projected points `radius` pixels away, gated by the disparity jump and the viewing angle.  One launch plus
// the clear of count:
//   normals_kernel   a block owns a tile of kNormalsTileH rows x kNormalsTileW columns of one pair.  It evaluates K15's z and the map's disparity d
//                    ONCE per pixel of the tile plus a halo of `radius` rows and columns (cloud_device.h: cloud_eval4d, 16-byte map loads where
//                    the alignment allows) into LDS, and every pixel takes its four neighbours from there.  A thread then owns four consecutive
//                    pixels of one row and stores them with raster_tiles.h's dense stores.
// The tile columns start ox % 4 pixels left of the image, as K15's groups do, so every group of four map pixels -- halo included -- is one aligned
// load that stays inside the padded row.  Pixels outside the H x W crop are never loaded and hold z = 0 in LDS: not kept, so never a neighbour.
// S2M2_NORMALS_LDS = 0 compiles the form without LDS instead: every pixel evaluates its four neighbours itself with per-pixel loads
// (profiles/normals/normalsbench.txt has both).  The arithmetic, and so every byte of the result, is the same.
#include "cloud_device.h"
#include "launch.h"
#include "plan.h"

#include <math.h>

#ifndef S2M2_NORMALS_LDS
#define S2M2_NORMALS_LDS 1
#endif

namespace s2m2 {

constexpr int kNormalsTileW = 64, kNormalsTileH = 16;    // 16 threads of four pixels x 16 rows = kRasterThreads
constexpr int kNormalsMaxRadius = 8;
constexpr int kNormalsLdsW = kNormalsTileW + 2 * kNormalsMaxRadius, kNormalsLdsH = kNormalsTileH + 2 * kNormalsMaxRadius;
static_assert(kNormalsTileW / 4 * kNormalsTileH == kRasterThreads, "one thread per group of four pixels");
static_assert(kNormalsMaxRadius % 4 == 0, "the halo columns are whole groups");

struct NormalsParams {
    CloudParams c;              // the inputs of K15 (its outputs are null; rows_per_tile / tiles are not used)
    float* depth;
    float* normals;
    unsigned char* image;
    int* count;
    int radius, tiles_x;        // the halo; tiles across a row (blockIdx.x = tile row * tiles_x + tile column)
    float gate, min_cos;
    int vec_depth, vec_normals, vec_image;   // depth / normals 16-byte aligned, image 4-byte aligned: dense_store4 may move a group whole
};

struct NormalsPoint {
    float x, y, z;
};

// a - b per component, a = the plus neighbour where it is usable, b = the minus neighbour where it is usable, else the centre: a central,
// forward or backward difference.  false: neither is usable
__device__ __forceinline__ bool normals_diff(const NormalsPoint& c, bool up, const NormalsPoint& plus, bool um, const NormalsPoint& minus, float (&d)[3]) {
#pragma clang fp contract(off)
    const NormalsPoint a = up ? plus : c, b = um ? minus : c;
    d[0] = a.x - b.x; d[1] = a.y - b.y; d[2] = a.z - b.z;
    return up || um;
}

// the unit normal of the pixel with the point c and the differences dx (horizontal) and dy (vertical): false = a hole (degenerate or grazing)
__device__ __forceinline__ bool normals_unit(const NormalsPoint& c, const float (&dx)[3], const float (&dy)[3], float min_cos, float (&n)[3]) {
#pragma clang fp contract(off)
    const float a0 = dy[1] * dx[2], b0 = dy[2] * dx[1];
    const float a1 = dy[2] * dx[0], b1 = dy[0] * dx[2];
    const float a2 = dy[0] * dx[1], b2 = dy[1] * dx[0];
    const float nx = a0 - b0, ny = a1 - b1, nz = a2 - b2;
    const float sx = nx * nx, sy = ny * ny, sz = nz * nz;
    const float sxy = sx + sy;
    const float s = sxy + sz;
    if (!(s > 0.f && s < INFINITY)) return false;
    const float q = sqrtf(s);
    n[0] = nx / q; n[1] = ny / q; n[2] = nz / q;
    const float mx = c.x * c.x, my = c.y * c.y, mz = c.z * c.z;
    const float mxy = mx + my;
    const float m = sqrtf(mxy + mz);
    const float tx = n[0] * c.x, ty = n[1] * c.y, tz = n[2] * c.z;
    const float txy = tx + ty;
    const float cosv = -((txy + tz) / m);
    return cosv >= min_cos;                                 // a NaN fails
}

__device__ __forceinline__ unsigned char normals_byte(float n) {
#pragma clang fp contract(off)
    const float s = n * 127.5f;
    return (unsigned char)(int)rintf(s + 127.5f);
}

#if !S2M2_NORMALS_LDS
// z and d of the image pixel (v, u), z = 0 outside the crop: the form without LDS
__device__ __forceinline__ void normals_eval1(const CloudParams& c, int b, int v, int u, float& z, float& d) {
    z = 0.f; d = 0.f;
    if (v < 0 || v >= c.H || u < 0 || u >= c.W) return;
    const size_t m = raster_map_index(c, b, v, u);
    d = c.disp[m];
    z = cloud_z(c, d, c.occ[m], c.conf[m]);
}
#endif

template <bool VEC>
__global__ __launch_bounds__(kRasterThreads) void normals_kernel(const NormalsParams p) {
    __shared__ int red[kRasterWaves];
    const CloudParams& c = p.c;
    const int b = blockIdx.y, r = p.radius;
    const int tile_y = (int)(blockIdx.x / (unsigned)p.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)p.tiles_x);
    const int v0 = tile_y * kNormalsTileH, c0 = -(c.ox & 3) + tile_x * kNormalsTileW;       // the tile's first row and column

#if S2M2_NORMALS_LDS
    // z and d of the tile and its halo: LDS row 0 is image row v0 - 8, LDS column 0 is image column c0 - 8; only the window the radius needs
    // is filled, in groups of four columns
    __shared__ __attribute__((aligned(16))) float zs[kNormalsLdsH][kNormalsLdsW];
    __shared__ __attribute__((aligned(16))) float ds[kNormalsLdsH][kNormalsLdsW];
    {
        const int hg = (r + 3) >> 2;                            // halo groups on either side
        const int ngx = kNormalsTileW / 4 + 2 * hg, nrows = kNormalsTileH + 2 * r;
        for (int i = threadIdx.x; i < ngx * nrows; i += kRasterThreads) {
            const int gy = i / ngx, gx = i - gy * ngx;
            const int ly = kNormalsMaxRadius - r + gy, lx = kNormalsMaxRadius - 4 * hg + 4 * gx;
            const int v = v0 - kNormalsMaxRadius + ly, u0 = c0 - kNormalsMaxRadius + lx;
            float z[4] = {0.f, 0.f, 0.f, 0.f}, d[4] = {0.f, 0.f, 0.f, 0.f};
            // a group with a pixel inside the crop: its map column ox + u0 is a multiple of four in [0, Wp), as K15's groups are
            if (v >= 0 && v < c.H && u0 + 3 >= 0 && u0 < c.W) cloud_eval4d<VEC>(c, b, v, u0, z, d);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                zs[ly][lx + j] = z[j];
                ds[ly][lx + j] = d[j];
            }
        }
    }
    __syncthreads();
#endif

    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int v = v0 + ty, u0 = c0 + tx * 4;
    int n_normals = 0;
    if (v < c.H && u0 < c.W) {                                  // u0 + 3 >= 0: c0 >= -3
        float depth[4], nrm[3][4];
        unsigned char col[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int u = u0 + j;
            depth[j] = 0.f;
#pragma unroll
            for (int a = 0; a < 3; ++a) { nrm[a][j] = 0.f; col[a][j] = 0; }
            if (u < 0 || u >= c.W) continue;
            // the centre and its four neighbours: z (0: not kept, also outside the crop) and d
            float zc, dc, zq[4], dq[4];
            const int qv[4] = {v, v, v + r, v - r}, qu[4] = {u + r, u - r, u, u};      // horizontal plus, minus; vertical plus, minus
#if S2M2_NORMALS_LDS
            const int ly = kNormalsMaxRadius + ty, lx = kNormalsMaxRadius + tx * 4 + j;
            zc = zs[ly][lx]; dc = ds[ly][lx];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                zq[k] = zs[ly + (qv[k] - v)][lx + (qu[k] - u)];
                dq[k] = ds[ly + (qv[k] - v)][lx + (qu[k] - u)];
            }
#else
            normals_eval1(c, b, v, u, zc, dc);
#pragma unroll
            for (int k = 0; k < 4; ++k) normals_eval1(c, b, qv[k], qu[k], zq[k], dq[k]);
#endif
            depth[j] = zc;
            if (!(zc > 0.f)) continue;
            NormalsPoint pc, pq[4];
            bool usable[4];
            pc.z = zc;
            cloud_xy(c, v, u, zc, pc.x, pc.y);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                usable[k] = zq[k] > 0.f && fabsf(dq[k] - dc) <= p.gate;               // a NaN fails
                pq[k].z = zq[k];
                cloud_xy(c, qv[k], qu[k], zq[k], pq[k].x, pq[k].y);
            }
            float dx[3], dy[3], n[3];
            const bool hx = normals_diff(pc, usable[0], pq[0], usable[1], pq[1], dx);
            const bool hy = normals_diff(pc, usable[2], pq[2], usable[3], pq[3], dy);
            if (!(hx && hy) || !normals_unit(pc, dx, dy, p.min_cos, n)) continue;
            ++n_normals;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                nrm[a][j] = n[a];
                col[a][j] = normals_byte(n[a]);
            }
        }
        const size_t plane = (size_t)c.H * c.W, line = (size_t)v * c.W;
        if (p.depth) dense_store4(p.depth, (size_t)b * plane + line, u0, c.W, p.vec_depth != 0, depth);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const size_t row = ((size_t)b * 3 + a) * plane + line;
            if (p.normals) dense_store4(p.normals, row, u0, c.W, p.vec_normals != 0, nrm[a]);
            if (p.image) dense_store4(p.image, row, u0, c.W, p.vec_image != 0, col[a]);
        }
    }
    if (p.count) {
        n_normals = block_sum_int(n_normals, red);
        if (threadIdx.x == 0 && n_normals) atomicAdd(p.count + b, n_normals);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host

static int normals_impl(const s2m2_normals_desc* d, void* stream) {
    S2M2_REQUIRE(d != nullptr, "normals: null descriptor");
    if (int rc = refuse_while_recording("normals")) return rc;
    NormalsParams p;
    bool vec = false;
    s2m2_cloud_desc in = d->cloud;                  // the inputs alone: the output fields of the embedded descriptor are ignored
    in.depth = nullptr; in.mask = nullptr; in.records = nullptr; in.count = nullptr; in.workspace = nullptr; in.capacity = 0;
    if (int rc = cloud_validate(&in, "normals", kCloudTilePixels, p.c, vec, false)) return rc;
    S2M2_REQUIRE(d->depth || d->normals || d->image || d->count,
                 "normals: no output requested (depth, normals, image and count are all null pointers)");
    S2M2_REQUIRE((((uintptr_t)d->depth | (uintptr_t)d->normals | (uintptr_t)d->count) & 3) == 0,
                 "normals: depth, normals and count must be 4-byte aligned");
    S2M2_REQUIRE(d->radius >= 1 && d->radius <= kNormalsMaxRadius, "normals: radius must be 1..%d (%d)", kNormalsMaxRadius, d->radius);
    S2M2_REQUIRE(d->max_jump >= 0.0, "normals: max_jump must be >= 0 (%g)", d->max_jump);                  // false for a NaN
    S2M2_REQUIRE(isfinite(d->min_cos) && d->min_cos < 1.0, "normals: min_cos must be finite and < 1 (%g)", d->min_cos);

    p.depth = d->depth; p.normals = d->normals; p.image = d->image; p.count = d->count;
    p.radius = d->radius;
    p.tiles_x = (int)(((long long)p.c.W + (p.c.ox & 3) + kNormalsTileW - 1) / kNormalsTileW);
    p.gate = (float)d->max_jump * (float)d->radius;
    p.min_cos = (float)d->min_cos;
    p.vec_depth = ((uintptr_t)d->depth & 15) == 0;
    p.vec_normals = ((uintptr_t)d->normals & 15) == 0;
    p.vec_image = ((uintptr_t)d->image & 3) == 0;

    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d->count && hipMemsetAsync(d->count, 0, sizeof(int) * (size_t)d->cloud.B, s) != hipSuccess) return set_error("normals: memset failed");
    const int tiles_y = (int)(((long long)p.c.H + kNormalsTileH - 1) / kNormalsTileH);
    const dim3 grid((unsigned)(p.tiles_x * tiles_y), d->cloud.B), block(kRasterThreads);       // tiles_x * tiles_y <= H * W < 2^31
    return vec ? launch<normals_kernel<true>>("normals", grid, block, 0, s, p) : launch<normals_kernel<false>>("normals", grid, block, 0, s, p);
}

}  // namespace s2m2

extern "C" int s2m2_normals(const s2m2_normals_desc* desc, void* stream) { return s2m2::normals_impl(desc, stream); }
