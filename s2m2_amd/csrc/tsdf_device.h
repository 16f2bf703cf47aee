// What K24's extraction (tsdf.hip: s2m2_tsdf_extract) and K25 (tsdf_mesh.hip: s2m2_tsdf_mesh) share: the extraction parameters, the predicate
// of a surface point (tsdf_crossings), the tile walk that counts the points and the one that ranks and stores them, and the host checks of the
// extraction descriptor.  K25's vertices are K24's points because both compile these functions.
#pragma once
#include "cloud_device.h"
#include "launch.h"
#include "plan.h"

#include <math.h>

namespace s2m2 {

constexpr int kTsdfTileVoxels = 8192;                    // voxels of one extraction tile (32 block steps)
constexpr long long kTsdfMaxVoxels = 1LL << 29;          // voxel indices, 3 points per voxel and 16 bytes per voxel from 32-bit indices

struct TsdfExtractParams {
    const uint4_t* volume;
    uint4_t* records;
    float* gradients;
    int* count;
    int* tile_counts;
    int Nx, Ny, Nz, n, tiles;   // n = Nx * Ny * Nz
    int min_weight;
    long long capacity;
    float gx, gy, gz, vs;
};

// tsdf and weight of voxel lin (the first 8 bytes of its record)
__device__ __forceinline__ void tsdf_tw(const TsdfExtractParams& p, int lin, float& t, int& w) {
    typedef unsigned uint2_t __attribute__((ext_vector_type(2)));
    const uint2_t o = *(const __attribute__((address_space(1))) uint2_t*)(p.volume + lin);
    t = __builtin_bit_cast(float, o[0]);
    w = (int)o[1];
}

// voxel lin = (i, j, k), lin < n: its tsdf t0, whether it is observed, and per axis a the tsdf t1[a] of the +1 neighbour and whether the pair
// (v0, v1) emits a point: v1 inside the grid and observed, and a sign change between them
__device__ __forceinline__ void tsdf_crossings(const TsdfExtractParams& p, int lin, int i, int j, int k, float& t0, float (&t1)[3], bool (&emit)[3]) {
    int w0;
    tsdf_tw(p, lin, t0, w0);
    const bool inside[3] = {i + 1 < p.Nx, j + 1 < p.Ny, k + 1 < p.Nz};
    const int step[3] = {1, p.Nx, p.Nx * p.Ny};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        emit[a] = false;
        t1[a] = 0.f;
        if (w0 >= p.min_weight && inside[a]) {
            int w1;
            tsdf_tw(p, lin + step[a], t1[a], w1);
            emit[a] = w1 >= p.min_weight && ((t0 < 0.f) != (t1[a] < 0.f));
        }
    }
}

// lin -> (i, j, k): 32-bit divisions (lin < 2^29)
__device__ __forceinline__ void tsdf_coords(const TsdfExtractParams& p, int lin, int& i, int& j, int& k) {
    const unsigned t = (unsigned)lin / (unsigned)p.Nx;
    i = lin - (int)t * p.Nx;
    k = (int)(t / (unsigned)p.Ny);
    j = (int)t - k * p.Ny;
}

// the surface points of voxel lin < n (0 .. 3)
__device__ __forceinline__ int tsdf_points_of(const TsdfExtractParams& p, int lin) {
    int i, j, k;
    tsdf_coords(p, lin, i, j, k);
    float t0, t1[3];
    bool emit[3];
    tsdf_crossings(p, lin, i, j, k, t0, t1, emit);
    return (int)emit[0] + (int)emit[1] + (int)emit[2];
}

// the tsdf of the neighbour of sel = (i, j, k) at distance `d` voxels along an axis (step = the axis' stride in voxels, pos / extent = sel's
// coordinate and the grid's size along it): the neighbour's where it is inside the grid and observed, ts otherwise
__device__ __forceinline__ float tsdf_neighbour(const TsdfExtractParams& p, int lin, int step, int pos, int extent, int d, float ts) {
    if (pos + d < 0 || pos + d >= extent) return ts;
    float t;
    int w;
    tsdf_tw(p, lin + d * step, t, w);
    return w >= p.min_weight ? t : ts;
}

// The store launch of a tile: K15's scatter -- tile_prefix, raster_rank_step with the three axis flags of a voxel, records and gradients.
// RANK_MAP (K25): rank_map[lin] takes the rank of voxel lin's first point (of the point it would emit next, where it emits none) for every
// voxel of the tile.  Block-uniform call; red: kRasterWaves ints of LDS, wave_n: 2 x kRasterWaves.
template <bool RANK_MAP>
__device__ __forceinline__ void tsdf_store_tile(const TsdfExtractParams& p, int* rank_map, int* red, int (*wave_n)[kRasterWaves]) {
#pragma clang fp contract(off)
    const int tile = blockIdx.x;
    long long base = tile_prefix(p.tile_counts, tile, red);
    const int first = tile * kTsdfTileVoxels, end = min(p.n, first + kTsdfTileVoxels);
    int step = 0;
    for (int lin0 = first; lin0 < end; lin0 += kRasterThreads) {        // block-uniform: every thread takes every step
        const int lin = lin0 + threadIdx.x;
        int i = 0, j = 0, k = 0;
        float t0 = 0.f, t1[3] = {0.f, 0.f, 0.f};
        bool emit[3] = {false, false, false};
        if (lin < end) {
            tsdf_coords(p, lin, i, j, k);
            tsdf_crossings(p, lin, i, j, k, t0, t1, emit);
        }
        long long r = raster_rank_step(emit, wave_n, step++, base);
        if constexpr (RANK_MAP) {
            if (lin < end) rank_map[lin] = (int)r;                       // 3 n < 2^31
        }
        const int stride[3] = {1, p.Nx, p.Nx * p.Ny};
        const int pos[3] = {i, j, k};
        const int extent[3] = {p.Nx, p.Ny, p.Nz};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!emit[a]) continue;
            if (r < p.capacity) {
                const float s = t0 / (t0 - t1[a]);
                float xyz[3] = {p.gx + (float)i * p.vs, p.gy + (float)j * p.vs, p.gz + (float)k * p.vs};
                xyz[a] = xyz[a] + s * p.vs;
                const bool far = fabsf(t1[a]) < fabsf(t0);               // sel = v1
                const int ls = far ? lin + stride[a] : lin;
                const float ts = far ? t1[a] : t0;
                if (p.records) {
                    const uint4_t o = *(const __attribute__((address_space(1))) uint4_t*)(p.volume + ls);
                    const unsigned cr = ((o[2] & 0xffffu) + 128u) >> 8, cg = ((o[2] >> 16) + 128u) >> 8, cb = ((o[3] & 0xffffu) + 128u) >> 8;
                    const uint4_t rec = {__builtin_bit_cast(unsigned, xyz[0]), __builtin_bit_cast(unsigned, xyz[1]), __builtin_bit_cast(unsigned, xyz[2]),
                                         cr | (cg << 8) | (cb << 16) | 0xff000000u};
                    p.records[r] = rec;
                }
                if (p.gradients) {
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        const int ps = pos[b] + (far && a == b ? 1 : 0);
                        const float tp = tsdf_neighbour(p, ls, stride[b], ps, extent[b], 1, ts);
                        const float tm = tsdf_neighbour(p, ls, stride[b], ps, extent[b], -1, ts);
                        p.gradients[(size_t)r * 3 + b] = tp - tm;
                    }
                }
            }
            ++r;
        }
    }
    if (p.count && tile == p.tiles - 1 && threadIdx.x == 0) *p.count = (int)base;
}

// ---------------------------------------------------------------------------------------------------------------- host

inline bool tsdf_finite_f32(double x) { return isfinite(x) && isfinite((float)x); }
inline bool tsdf_positive_f32(double x) { return tsdf_finite_f32(x) && x > 0.0 && (float)x > 0.f; }

inline bool tsdf_dims_ok(int Nx, int Ny, int Nz) {
    return Nx > 0 && Ny > 0 && Nz > 0 && (long long)Nx * Ny < kTsdfMaxVoxels && (long long)Nx * Ny * Nz < kTsdfMaxVoxels;
}

// the checks that every entry point makes of a volume: the buffer, the dims, the grid's placement
inline int tsdf_check_volume(const char* what, const void* volume, int Nx, int Ny, int Nz, const double* origin, double voxel_size) {
    S2M2_REQUIRE(volume != nullptr, "%s: null pointer (volume)", what);
    S2M2_REQUIRE(((uintptr_t)volume & 15) == 0, "%s: the volume must be 16-byte aligned", what);
    S2M2_REQUIRE(Nx > 0 && Ny > 0 && Nz > 0, "%s: non-positive dims Nx=%d Ny=%d Nz=%d", what, Nx, Ny, Nz);
    S2M2_REQUIRE(tsdf_dims_ok(Nx, Ny, Nz), "%s: dims too large (Nx*Ny*Nz < 2^29)", what);
    S2M2_REQUIRE(tsdf_positive_f32(voxel_size), "%s: voxel_size must be finite and > 0 in fp32 (%g)", what, voxel_size);
    S2M2_REQUIRE(tsdf_finite_f32(origin[0]) && tsdf_finite_f32(origin[1]) && tsdf_finite_f32(origin[2]), "%s: the origin must be finite (also in fp32)", what);
    return 0;
}

// the checks of an extraction descriptor but for its workspace (`need_output`: records, gradients and count may not all be NULL), and the
// kernels' parameters from it (tile_counts is left to the caller)
inline int tsdf_extract_params(const char* what, const s2m2_tsdf_extract_desc* d, bool need_output, TsdfExtractParams& p) {
    if (int rc = tsdf_check_volume(what, d->volume, d->Nx, d->Ny, d->Nz, d->origin, d->voxel_size)) return rc;
    S2M2_REQUIRE(d->min_weight >= 1, "%s: min_weight must be >= 1 (%d)", what, d->min_weight);
    S2M2_REQUIRE(!need_output || d->records || d->gradients || d->count, "%s: no output requested (records, gradients and count are all null pointers)", what);
    S2M2_REQUIRE(d->capacity >= 0, "%s: negative capacity %lld", what, d->capacity);
    S2M2_REQUIRE(d->records || d->gradients || d->capacity == 0, "%s: null pointers (records and gradients) with capacity %lld", what, d->capacity);
    S2M2_REQUIRE(((uintptr_t)d->records & 15) == 0, "%s: records must be 16-byte aligned", what);
    S2M2_REQUIRE((((uintptr_t)d->gradients | (uintptr_t)d->count) & 3) == 0, "%s: gradients and count must be 4-byte aligned", what);
    p.volume = static_cast<const uint4_t*>(d->volume);
    p.records = static_cast<uint4_t*>(d->records);
    p.gradients = d->gradients;
    p.count = d->count;
    p.tile_counts = nullptr;
    p.Nx = d->Nx; p.Ny = d->Ny; p.Nz = d->Nz;
    p.n = d->Nx * d->Ny * d->Nz;
    p.tiles = (p.n + kTsdfTileVoxels - 1) / kTsdfTileVoxels;
    p.min_weight = d->min_weight;
    p.capacity = d->capacity;
    p.gx = (float)d->origin[0]; p.gy = (float)d->origin[1]; p.gz = (float)d->origin[2];
    p.vs = (float)d->voxel_size;
    return 0;
}

}  // namespace s2m2
