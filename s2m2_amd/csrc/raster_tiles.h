// The raster tile walk of the output stages K15 (cloud.hip), K18 (evalstats.hip) and K20 (mesh.hip): the pixel -> thread map, the loads and
// stores of a thread's four pixels, the block reductions and the raster-order rank step.  What a stage computes per pixel is not here
// (cloud_device.h for K15 / K20, evalstats.hip for K18).
// A block owns a tile of whole rows of one pair (raster_host.h: tile_rows) and walks it in block steps of kRasterChunk pixels, row by row, left
// to right.  Pixel -> thread map: a thread owns four consecutive pixels of one row, placed so that their MAP column is a multiple of four
// whatever the crop offset is (the first group of a row starts ox % 4 pixels left of the image): with Wp % 4 == 0 every map read is one aligned
// 16-byte load that stays inside the padded row.  The unpadded (B, H, W) tensors follow their own rows: a group is moved whole where its element
// index is a multiple of four and the tensor's base is aligned, per pixel otherwise.
// The parameter structs of the stages name the geometry alike (H, W, Hp, Wp, oy, ox, rows_per_tile): the helpers take them as `P`.
#pragma once
#include "common.h"
#include "raster_host.h"

namespace s2m2 {

constexpr int kRasterThreads = 256;                      // four waves
constexpr int kRasterWaves = kRasterThreads / 64;
constexpr int kRasterChunk = kRasterThreads * 4;         // pixels of one block step

// The block-uniform walk over rows [tile * rows_per_tile, min(v_limit, (tile + 1) * rows_per_tile)) in block steps:
//     for (RasterWalk w(p, tile, p.H); w.more(); w.next()) { row w.v, this thread's first column w.u0() }
// Every thread takes every step -- also those whose group lies beyond the row (u0 >= W) --, so the body may hold barriers and shuffles.  A copy
// advanced by next() names the step after, which lets K18 issue that step's loads ahead (eval_tile_kernel).
struct RasterWalk {
    int v, c0;                  // image row; first column of the block step: -(ox & 3) + k * kRasterChunk
    int v_end, W, shift;
    template <typename P>
    __device__ __forceinline__ RasterWalk(const P& p, int tile, int v_limit)
        : v(tile * p.rows_per_tile), c0(-(p.ox & 3)), v_end(min(v_limit, (tile + 1) * p.rows_per_tile)), W(p.W), shift(p.ox & 3) {}
    __device__ __forceinline__ bool more() const { return v < v_end; }
    // first image column of this thread's group (may be < 0 in the first step of a row, and reach beyond W in the last)
    __device__ __forceinline__ int u0() const { return c0 + (int)threadIdx.x * 4; }
    __device__ __forceinline__ void next() {
        c0 += kRasterChunk;
        if (c0 >= W) { c0 = -shift; ++v; }
    }
};

// element index of image column u of row v of pair b in the padded maps (p.ox + u >= 0 by construction, also for the u0 < 0 of a row's first
// group), and of image column 0 in the unpadded tensors
template <typename P> __device__ __forceinline__ size_t raster_map_index(const P& p, int b, int v, int u) {
    return ((size_t)b * p.Hp + (v + p.oy)) * (size_t)p.Wp + (size_t)(p.ox + u);
}
template <typename P> __device__ __forceinline__ size_t raster_dense_row(const P& p, int b, int v) { return ((size_t)b * p.H + v) * (size_t)p.W; }

// Four consecutive fp32 values of a padded map row, image columns u0 .. u0 + 3 (m: raster_map_index of u0).  VEC: one 16-byte load, aligned and
// inside the padded row (see the head of the file); else per pixel, 0 for the pixels outside [0, W).
template <bool VEC>
__device__ __forceinline__ void map_load4(const float* map, size_t m, int u0, int W, float x[4]) {
    if constexpr (VEC) {
        const raw16_t v = global_load16(map + m);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = v[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = (u0 + j >= 0 && u0 + j < W) ? map[m + j] : 0.f;
    }
}

// The same four pixels in a row of an unpadded tensor of float, int or unsigned char (row: raster_dense_row; row + u0 wraps for u0 < 0 and is
// only used where the pixel exists).  `aligned`: the tensor's base is aligned to four elements, so a group inside [0, W) whose element index is
// a multiple of four is one aligned 16-byte / 4-byte access.  Everything else goes per pixel inside [0, W); a load leaves the other x alone.
__device__ __forceinline__ bool dense_whole(size_t row, int u0, int W) { return u0 >= 0 && u0 + 3 < W && ((row + u0) & 3) == 0; }

template <typename T>
__device__ __forceinline__ void dense_store4(T* t, size_t row, int u0, int W, bool aligned, const T x[4]) {
    typedef T vec4 __attribute__((ext_vector_type(4)));
    if (aligned && dense_whole(row, u0, W)) {
        const vec4 v = {x[0], x[1], x[2], x[3]};
        *reinterpret_cast<vec4*>(t + row + u0) = v;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (u0 + j >= 0 && u0 + j < W) t[row + u0 + j] = x[j];
    }
}

template <typename T>
__device__ __forceinline__ void dense_load4(const T* t, size_t row, int u0, int W, bool aligned, T x[4]) {
    typedef T vec4 __attribute__((ext_vector_type(4)));
    if (aligned && dense_whole(row, u0, W)) {
        const vec4 v = *(const __attribute__((address_space(1))) vec4*)(t + row + u0);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = v[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (u0 + j >= 0 && u0 + j < W) x[j] = t[row + u0 + j];
    }
}

// the validity filter of include/s2m2_hip.h: the `valid` half of K15's keep (cloud_device.h: cloud_z) and K18's KEPT set
__device__ __forceinline__ bool cloud_valid(float conf, float occ, float conf_min, float occ_min) { return conf > conf_min && occ > occ_min; }

__device__ __forceinline__ int wave_sum_int(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// sum over the block of one int per thread, result in every thread (red: kRasterWaves ints of LDS, not reused before the next barrier)
__device__ __forceinline__ int block_sum_int(int x, int* red) {
    x = wave_sum_int(x);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < kRasterWaves; ++w) s += red[w];
    return s;
}

// items of this pair in the tiles before `tile` (counts: one int per tile, written by the stage's count launch): strided over the block, then
// block_sum_int
__device__ __forceinline__ int tile_prefix(const int* counts, int tile, int* red) {
    int before = 0;
    for (int t = threadIdx.x; t < tile; t += kRasterThreads) before += counts[t];
    return block_sum_int(before, red);
}

// One block step of the raster-order ranks.  Every thread holds NF flags in raster order; the items run by wave, then by lane, then by flag.
// Returns the rank of this thread's first flagged item -- its later ones follow back to back -- and advances `base` (the items before this
// step) by the block's total.  Inside the wave: the flagged items of the lanes below come first (ballots + mbcnt).  Across the four waves: the
// wave totals meet in wave_n[step & 1] behind ONE barrier.  Two buffers make that enough: a wave that is a step ahead writes the other buffer,
// and the step after next rewrites this one only behind the next step's barrier, which no wave passes before every wave has read its totals
// here.  Block-uniform call with a block-uniform `step` that counts the calls.
template <int NF>
__device__ __forceinline__ long long raster_rank_step(const bool (&flags)[NF], int (*wave_n)[kRasterWaves], int step, long long& base) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int below = 0, wave_total = 0;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const unsigned long long bal = __ballot(flags[j]);
        below += __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
        wave_total += __popcll(bal);
    }
    if (lane == 0) wave_n[step & 1][wave] = wave_total;
    __syncthreads();
    long long r = base;
    int block_total = 0;
#pragma unroll
    for (int w = 0; w < kRasterWaves; ++w) {
        const int nw = wave_n[step & 1][w];
        if (w < wave) r += nw;
        block_total += nw;
    }
    base += block_total;
    return r + below;
}

}  // namespace s2m2
