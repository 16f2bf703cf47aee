// K15: the 3D output stage behind the forward (include/s2m2_hip.h: s2m2_cloud) -- validity filter, metric depth, and the kept pixels compacted
// into a coloured point cloud in raster order.  Two launches without a host step, atomics or waiting between blocks:
//   cloud_count_kernel    a block owns a tile of whole image rows: dense depth / mask, one count per tile into the workspace
//   cloud_scatter_kernel  a block sums the counts of the tiles before its own (tile_prefix), recomputes keep, ranks its pixels
//                         (raster_rank_step) and stores the records; with RANK (K20's vertex launch) also the rank of every pixel
// The per-pixel chain and the record live in cloud_device.h, which K20 (mesh.hip) compiles as well; the tile walk, the loads and stores of a
// thread's four pixels and the rank step in raster_tiles.h.  Image reads follow the unpadded rows and are per pixel.
#include "cloud_device.h"
#include "launch.h"
#include "plan.h"

#include <type_traits>

namespace s2m2 {

template <bool VEC>
__global__ __launch_bounds__(kRasterThreads) void cloud_count_kernel(const CloudParams p) {
    __shared__ int red[kRasterWaves];
    const int b = blockIdx.y, tile = blockIdx.x;
    int n = 0;
    for (RasterWalk w(p, tile, p.H); w.more(); w.next()) {
        const int v = w.v, u0 = w.u0();
        if (u0 >= p.W) continue;
        float z[4];
        cloud_eval4<VEC>(p, b, v, u0, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) n += z[j] > 0.f;
        cloud_store_dense<VEC>(p, b, v, u0, z);
    }
    if (p.tile_counts) {
        n = block_sum_int(n, red);
        if (threadIdx.x == 0) p.tile_counts[(size_t)b * p.tiles + tile] = n;
    }
}

// K15 launches RANK = false on its CloudParams.  K20's vertex launch is RANK = true on its MeshParams (mesh_vertices below): the same records,
// and the rank of every pixel (-1: not kept) into the dense rank map.
template <bool RANK> using ScatterParams = std::conditional_t<RANK, MeshParams, CloudParams>;
__device__ __forceinline__ const CloudParams& cloud_of(const CloudParams& p) { return p; }
__device__ __forceinline__ const CloudParams& cloud_of(const MeshParams& mp) { return mp.c; }

template <bool VEC, typename IT, bool RANK>
__global__ __launch_bounds__(kRasterThreads) void cloud_scatter_kernel(const ScatterParams<RANK> pp) {
    __shared__ int red[kRasterWaves];
    __shared__ int wave_n[2][kRasterWaves];
    const CloudParams& p = cloud_of(pp);
    const int b = blockIdx.y, tile = blockIdx.x;
    long long base = tile_prefix(p.tile_counts + (size_t)b * p.tiles, tile, red);      // kept pixels of this pair in the tiles before this one
    const IT* img = static_cast<const IT*>(p.image) + (size_t)b * 3 * p.H * p.W;
    const size_t plane = (size_t)p.H * p.W;
    uint4_t* rec = p.records + (size_t)b * (size_t)p.capacity;
    int step = 0;
    for (RasterWalk w(p, tile, p.H); w.more(); w.next()) {
        const int v = w.v, u0 = w.u0();
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (u0 < p.W) cloud_eval4<VEC>(p, b, v, u0, z);
        const bool keep[4] = {z[0] > 0.f, z[1] > 0.f, z[2] > 0.f, z[3] > 0.f};
        long long r = raster_rank_step(keep, wave_n, step++, base);
        int rk[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            rk[j] = -1;
            if (keep[j]) {
                if (r < p.capacity) rec[r] = cloud_record<IT>(p, img, plane, v, u0 + j, z[j]);
                rk[j] = (int)r;
                ++r;
            }
        }
        if constexpr (RANK) {
            if (u0 < p.W) dense_store4(pp.rank, raster_dense_row(p, b, v), u0, p.W, pp.rank_vec != 0, rk);
        }
    }
    if (tile == p.tiles - 1 && threadIdx.x == 0) p.count[b] = (int)base;
}

// every check of a s2m2_cloud_desc that include/s2m2_hip.h lists, then the kernel parameters: shared with s2m2_mesh (mesh.hip), which takes the
// same descriptor fields (`what` prefixes the messages) with its own tile size.  K21 (register.hip) reads the inputs alone and has outputs of its
// own: it passes a copy without the output fields and outputs = false
int cloud_validate(const s2m2_cloud_desc* d, const char* what, int tile_pixels, CloudParams& p, bool& vec, bool outputs) {
    S2M2_REQUIRE(d->disp && d->occ && d->conf, "%s: null pointer (disp / occ / conf)", what);
    S2M2_REQUIRE(!outputs || d->depth || d->mask || d->count, "%s: no output requested (depth, mask and count are all null pointers)", what);
    if (int rc = check_padded_maps(what, "image", d->B, d->H, d->W, d->Hp, d->Wp)) return rc;
    S2M2_REQUIRE(d->fx > 0.0 && d->fy > 0.0, "%s: fx and fy must be positive (fx=%g fy=%g)", what, d->fx, d->fy);
    S2M2_REQUIRE(d->depth_scale > 0.0, "%s: depth_scale must be positive (%g)", what, d->depth_scale);
    S2M2_REQUIRE(d->capacity >= 0, "%s: negative capacity %lld", what, d->capacity);
    S2M2_REQUIRE(d->image_dtype == S2M2_F32 || d->image_dtype == S2M2_F16 || d->image_dtype == 2, "%s: unsupported image dtype %d", what,
                 d->image_dtype);
    if (d->count) {
        S2M2_REQUIRE(d->image != nullptr, "%s: null pointer (image) while a cloud is requested", what);
        S2M2_REQUIRE(d->workspace != nullptr, "%s: null workspace while a cloud is requested (s2m2_%s_workspace_bytes)", what, what);
        S2M2_REQUIRE(((uintptr_t)d->workspace & 3) == 0, "%s: the workspace must be 4-byte aligned", what);
        S2M2_REQUIRE(d->records != nullptr || d->capacity == 0, "%s: null pointer (records) with capacity %lld", what, d->capacity);
        S2M2_REQUIRE(((uintptr_t)d->records & 15) == 0, "%s: records must be 16-byte aligned", what);
    }
    S2M2_REQUIRE(((uintptr_t)d->depth & 3) == 0 && ((uintptr_t)d->disp & 3) == 0 && ((uintptr_t)d->occ & 3) == 0 && ((uintptr_t)d->conf & 3) == 0,
                 "%s: fp32 tensors must be 4-byte aligned", what);

    p.disp = d->disp; p.occ = d->occ; p.conf = d->conf; p.image = d->image;
    p.depth = d->depth; p.mask = d->mask;
    p.records = static_cast<uint4_t*>(d->records);
    p.count = d->count;
    p.tile_counts = d->count ? static_cast<int*>(d->workspace) : nullptr;
    p.H = d->H; p.W = d->W; p.Hp = d->Hp; p.Wp = d->Wp;
    p.oy = (d->Hp - d->H) / 2; p.ox = (d->Wp - d->W) / 2;
    p.rows_per_tile = tile_rows(d->W, tile_pixels);
    p.tiles = tiles(d->H, p.rows_per_tile);
    p.unfiltered = d->unfiltered != 0;
    p.capacity = d->capacity;
    p.bf = (float)(d->baseline * d->fx);
    p.doffs = (float)d->doffs;
    p.depth_scale = (float)d->depth_scale;
    p.depth_trunc = d->depth_trunc > 0.0 ? (float)d->depth_trunc : 1e9f;
    p.conf_min = (float)d->conf_min; p.occ_min = (float)d->occ_min;
    p.fx = (float)d->fx; p.fy = (float)d->fy; p.cx = (float)d->cx; p.cy = (float)d->cy;
    S2M2_REQUIRE(p.fx > 0.f && p.fy > 0.f && p.depth_scale > 0.f, "%s: fx, fy and depth_scale must be positive in fp32", what);
    // the aligned form: 16-byte map loads.  The dense outputs take 16-byte / 4-byte group stores only where their own address allows it
    // (checked per group in the kernel against the element index: that needs the base pointers aligned too, else the per-pixel form)
    vec = d->Wp % 4 == 0 && (((uintptr_t)d->disp | (uintptr_t)d->occ | (uintptr_t)d->conf) & 15) == 0 && ((uintptr_t)d->depth & 15) == 0 &&
          ((uintptr_t)d->mask & 3) == 0;
    return 0;
}

// the scatter launch of K15 (`what` = "cloud (scatter)") and of K20 ("mesh (vertices)"); the image dtype is validated by cloud_validate
template <bool RANK>
static int cloud_scatter(const char* entry, const char* what, const ScatterParams<RANK>& pp, bool vec, int image_dtype, dim3 grid, hipStream_t s) {
    return by_image_dtype(image_dtype, entry, [&](auto ti) {
        using IT = decltype(ti);
        if (vec) return launch<cloud_scatter_kernel<true, IT, RANK>>(what, grid, dim3(kRasterThreads), 0, s, pp);
        return launch<cloud_scatter_kernel<false, IT, RANK>>(what, grid, dim3(kRasterThreads), 0, s, pp);
    });
}

int mesh_vertices(const MeshParams& mp, bool vec, int image_dtype, dim3 grid, hipStream_t s) {
    return cloud_scatter<true>("mesh", "mesh (vertices)", mp, vec, image_dtype, grid, s);
}

static int cloud_impl(const s2m2_cloud_desc* d, void* stream) {
    S2M2_REQUIRE(d != nullptr, "cloud: null descriptor");
    if (int rc = refuse_while_recording("cloud")) return rc;
    CloudParams p;
    bool vec = false;
    if (int rc = cloud_validate(d, "cloud", kCloudTilePixels, p, vec)) return rc;
    const dim3 grid(p.tiles, d->B), block(kRasterThreads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = vec ? launch<cloud_count_kernel<true>>("cloud (count)", grid, block, 0, s, p) : launch<cloud_count_kernel<false>>("cloud (count)", grid, block, 0, s, p))
        return rc;
    if (!d->count) return 0;
    return cloud_scatter<false>("cloud", "cloud (scatter)", p, vec, d->image_dtype, grid, s);
}

}  // namespace s2m2

extern "C" size_t s2m2_cloud_workspace_bytes(int B, int H, int W) {
    using namespace s2m2;
    if (!raster_extents_ok(B, H, W)) return 0;
    return round256((size_t)B * tiles(H, tile_rows(W, kCloudTilePixels)) * sizeof(int));
}

extern "C" int s2m2_cloud(const s2m2_cloud_desc* desc, void* stream) { return s2m2::cloud_impl(desc, stream); }
