// Device functions shared by K15 (cloud.hip) and K20 (mesh.hip): the per-pixel chain of include/s2m2_hip.h (keep, z, x, y, colour bytes), the
// pixel -> thread map and the block reductions.  Both kernels compile THESE functions, so that the vertex records of s2m2_mesh are byte-identical
// to the records of s2m2_cloud whatever the compiler does with the arithmetic.
// Pixel -> thread map: a thread owns four consecutive pixels of one row, placed so that their MAP column is a multiple of four whatever the crop
// offset is (the first group of a row starts (Wp-W)/2 % 4 pixels left of the image): with Wp % 4 == 0 every map read is one aligned 16-byte
// load that stays inside the padded row.
#pragma once
#include "common.h"

namespace s2m2 {

constexpr int kCloudThreads = 256;                       // four waves
constexpr int kCloudChunk = kCloudThreads * 4;           // pixels of one block step
constexpr int kCloudTilePixels = 4096;                   // a tile: as many whole rows as fit (at least one)

static inline int cloud_tile_rows(int W) { return W >= kCloudTilePixels ? 1 : kCloudTilePixels / W; }

typedef unsigned uint4_t __attribute__((ext_vector_type(4)));
typedef unsigned char uchar4_t __attribute__((ext_vector_type(4)));

struct CloudParams {
    const float* disp;
    const float* occ;
    const float* conf;
    const void* image;
    float* depth;
    unsigned char* mask;
    uint4_t* records;
    int* count;
    int* tile_counts;
    int H, W, Hp, Wp;
    int oy, ox;                 // crop offsets
    int rows_per_tile, tiles;   // tiles per pair
    int unfiltered;
    long long capacity;
    float bf, doffs, depth_scale, depth_trunc, conf_min, occ_min;
    float fx, fy, cx, cy;
};

// z of one pixel, or 0 when it is not kept (keep <=> z > 0): the arithmetic of the header, one fp32 rounding per operation
__device__ __forceinline__ float cloud_z(const CloudParams& p, float disp, float occ, float conf) {
    const bool valid = p.unfiltered || (conf > p.conf_min && occ > p.occ_min);
    const float d = valid ? disp : -1.f;
    const float depth = d <= 0.f ? 1e9f : p.bf / (d + p.doffs);
    const float z = depth / p.depth_scale;
    return (z > 0.f && z < p.depth_trunc) ? z : 0.f;
}

// the four pixels of this thread in image row v, first column u0 (may be < 0 or reach beyond W: those pixels give z = 0, d = 0): z and the
// map's disparity d
template <bool VEC>
__device__ __forceinline__ void cloud_eval4d(const CloudParams& p, int b, int v, int u0, float z[4], float d[4]) {
    const size_t m = ((size_t)b * p.Hp + (v + p.oy)) * (size_t)p.Wp + (size_t)(p.ox + u0);      // p.ox + u0 >= 0 by construction
    float o[4], c[4];
    if constexpr (VEC) {                                 // aligned and inside the padded row: see the head of the file
        const raw16_t dv = global_load16(p.disp + m), ov = global_load16(p.occ + m), cv = global_load16(p.conf + m);
#pragma unroll
        for (int j = 0; j < 4; ++j) { d[j] = dv[j]; o[j] = ov[j]; c[j] = cv[j]; }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = u0 + j >= 0 && u0 + j < p.W;
            d[j] = in ? p.disp[m + j] : 0.f;
            o[j] = in ? p.occ[m + j] : 0.f;
            c[j] = in ? p.conf[m + j] : 0.f;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = (u0 + j >= 0 && u0 + j < p.W) ? cloud_z(p, d[j], o[j], c[j]) : 0.f;
}

template <bool VEC>
__device__ __forceinline__ void cloud_eval4(const CloudParams& p, int b, int v, int u0, float z[4]) {
    float d[4];
    cloud_eval4d<VEC>(p, b, v, u0, z, d);
}

template <typename IT> __device__ __forceinline__ unsigned cloud_byte(IT x);
template <> __device__ __forceinline__ unsigned cloud_byte<unsigned char>(unsigned char x) { return x; }
template <> __device__ __forceinline__ unsigned cloud_byte<float>(float x) { return (unsigned)__float2int_rn(fminf(fmaxf(x, 0.f), 255.f)); }
template <> __device__ __forceinline__ unsigned cloud_byte<half_t>(half_t x) { return cloud_byte<float>((float)x); }

// the 16-byte record of the kept pixel (v, u) of one pair: img = the pair's planar image, plane = H * W, z = the pixel's z
template <typename IT>
__device__ __forceinline__ uint4_t cloud_record(const CloudParams& p, const IT* img, size_t plane, int v, int u, float z) {
    const size_t px = (size_t)v * p.W + u;
    const unsigned cr = cloud_byte<IT>(img[px]), cg = cloud_byte<IT>(img[plane + px]), cb = cloud_byte<IT>(img[2 * plane + px]);
    const float fv = (float)v - p.cy;
    const float x = ((float)u - p.cx) * z / p.fx;
    const float y = fv * z / p.fy;
    uint4_t o = {__builtin_bit_cast(unsigned, x), __builtin_bit_cast(unsigned, y), __builtin_bit_cast(unsigned, z),
                 cr | (cg << 8) | (cb << 16) | 0xff000000u};
    return o;
}

__device__ __forceinline__ int wave_sum_int(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// sum over the block of one int per thread, result in every thread (red: kCloudThreads / 64 ints of LDS, not reused before the next barrier)
__device__ __forceinline__ int block_sum_int(int x, int* red) {
    x = wave_sum_int(x);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < kCloudThreads / 64; ++w) s += red[w];
    return s;
}

// the header's checks of a s2m2_cloud_desc, shared by s2m2_cloud and s2m2_mesh (`what` prefixes the messages); fills p
int cloud_validate(const s2m2_cloud_desc* d, const char* what, CloudParams& p, bool& vec);

static inline bool cloud_extents_ok(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 31) && B <= 65535;
}

}  // namespace s2m2
