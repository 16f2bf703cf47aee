// Device functions shared by K15 (cloud.hip), K20 (mesh.hip) and K23 (voxel.hip): the per-pixel chain of include/s2m2_hip.h (keep, z, x, y,
// colour bytes) and the record.  All three compile THESE functions, so that the vertex records of s2m2_mesh are byte-identical to the records
// of s2m2_cloud, and the points s2m2_voxel sums are K15's, whatever the compiler does with the arithmetic.  The pixel -> thread map, the loads
// and stores of a thread's four pixels, the block reductions and the rank step are raster_tiles.h's, which K18 shares.
#pragma once
#include "raster_tiles.h"

namespace s2m2 {

constexpr int kCloudTilePixels = 4096;                   // K15's tile (raster_host.h: tile_rows)

typedef unsigned uint4_t __attribute__((ext_vector_type(4)));

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
    const bool valid = p.unfiltered || cloud_valid(conf, occ, p.conf_min, p.occ_min);
    const float d = valid ? disp : -1.f;
    const float depth = d <= 0.f ? 1e9f : p.bf / (d + p.doffs);
    const float z = depth / p.depth_scale;
    return (z > 0.f && z < p.depth_trunc) ? z : 0.f;
}

// the four pixels of this thread in image row v, first column u0 (may be < 0 or reach beyond W: those pixels give z = 0, d = 0): z and the
// map's disparity d
template <bool VEC>
__device__ __forceinline__ void cloud_eval4d(const CloudParams& p, int b, int v, int u0, float z[4], float d[4]) {
    const size_t m = raster_map_index(p, b, v, u0);
    float o[4], c[4];
    map_load4<VEC>(p.disp, m, u0, p.W, d);
    map_load4<VEC>(p.occ, m, u0, p.W, o);
    map_load4<VEC>(p.conf, m, u0, p.W, c);
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

// x and y of the kept pixel (v, u) at depth z, and its colour bytes (img = the pair's planar image, plane = H * W): the arithmetic of the
// record, which K23 (voxel.hip) quantises and sums instead of storing
__device__ __forceinline__ void cloud_xy(const CloudParams& p, int v, int u, float z, float& x, float& y) {
    const float fv = (float)v - p.cy;
    x = ((float)u - p.cx) * z / p.fx;
    y = fv * z / p.fy;
}
template <typename IT>
__device__ __forceinline__ void cloud_colour(const CloudParams& p, const IT* img, size_t plane, int v, int u, unsigned& cr, unsigned& cg, unsigned& cb) {
    const size_t px = (size_t)v * p.W + u;
    cr = cloud_byte<IT>(img[px]); cg = cloud_byte<IT>(img[plane + px]); cb = cloud_byte<IT>(img[2 * plane + px]);
}

// the 16-byte record of the kept pixel (v, u) of one pair, z = the pixel's z
template <typename IT>
__device__ __forceinline__ uint4_t cloud_record(const CloudParams& p, const IT* img, size_t plane, int v, int u, float z) {
    unsigned cr, cg, cb;
    cloud_colour<IT>(p, img, plane, v, u, cr, cg, cb);
    float x, y;
    cloud_xy(p, v, u, z, x, y);
    uint4_t o = {__builtin_bit_cast(unsigned, x), __builtin_bit_cast(unsigned, y), __builtin_bit_cast(unsigned, z),
                 cr | (cg << 8) | (cb << 16) | 0xff000000u};
    return o;
}

// The dense outputs of the count launches of K15 and K20: z and keep of the thread's four pixels of row v (u0 < W).  VEC carries the alignment
// of both bases (cloud_validate).
template <bool VEC>
__device__ __forceinline__ void cloud_store_dense(const CloudParams& p, int b, int v, int u0, const float z[4]) {
    const size_t row = raster_dense_row(p, b, v);
    if (p.depth) dense_store4(p.depth, row, u0, p.W, VEC, z);
    if (p.mask) {
        const unsigned char k[4] = {(unsigned char)(z[0] > 0.f), (unsigned char)(z[1] > 0.f), (unsigned char)(z[2] > 0.f), (unsigned char)(z[3] > 0.f)};
        dense_store4(p.mask, row, u0, p.W, VEC, k);
    }
}

// K20's parameters: K15's, the faces and the dense rank map that K15's scatter kernel fills for it
struct MeshParams {
    CloudParams c;
    int* faces;                 // (B, face_capacity, 3)
    int* face_count;
    int* rank;                  // (B, H, W): the dense rank map
    int* tile_faces;            // faces per tile, behind the vertex counts in the workspace
    long long face_capacity;
    float max_jump;
    int rank_vec;               // the rank map is 16-byte aligned: aligned groups of four take one load / store
};

// cloud.hip.  The header's checks of a s2m2_cloud_desc, shared by s2m2_cloud and s2m2_mesh (`what` prefixes the messages); fills p, with the
// tile geometry of tile_pixels.  outputs = false (K21): the descriptor need not request an output
int cloud_validate(const s2m2_cloud_desc* d, const char* what, int tile_pixels, CloudParams& p, bool& vec, bool outputs = true);
// K20's vertex launch: cloud_scatter_kernel with the rank-map option on mp's tile geometry
int mesh_vertices(const MeshParams& mp, bool vec, int image_dtype, dim3 grid, hipStream_t stream);

}  // namespace s2m2
