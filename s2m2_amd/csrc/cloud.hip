// K15: the 3D output stage behind the forward (include/s2m2_hip.h: s2m2_cloud) -- validity filter, metric depth, and the kept pixels compacted
// into a coloured point cloud in raster order.  Two launches without a host step, atomics or waiting between blocks:
//   cloud_count_kernel    a block owns a tile of whole image rows: dense depth / mask, one count per tile into the workspace
//   cloud_scatter_kernel  a block sums the counts of the tiles before its own (strided over the block, wave + block reduction), recomputes
//                         keep, ranks its pixels (wave ballots + mbcnt, a prefix over the four waves through LDS) and stores the records
// The per-pixel chain, the pixel -> thread map and the record live in cloud_device.h, which K20 (mesh.hip) compiles as well.  Image reads and
// the dense stores follow the unpadded rows and are per pixel unless a group is aligned.
#include "cloud_device.h"
#include "launch.h"
#include "plan.h"

namespace s2m2 {

template <bool VEC>
__global__ __launch_bounds__(kCloudThreads) void cloud_count_kernel(const CloudParams p) {
    __shared__ int red[kCloudThreads / 64];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int shift = p.ox & 3;
    const int v_end = min(p.H, (tile + 1) * p.rows_per_tile);
    int n = 0;
    for (int v = tile * p.rows_per_tile; v < v_end; ++v) {
        const size_t row = ((size_t)b * p.H + v) * (size_t)p.W;
        for (int u0 = (int)threadIdx.x * 4 - shift; u0 < p.W; u0 += kCloudChunk) {
            float z[4];
            cloud_eval4<VEC>(p, b, v, u0, z);
#pragma unroll
            for (int j = 0; j < 4; ++j) n += z[j] > 0.f;
            const bool whole = VEC && u0 >= 0 && u0 + 3 < p.W && ((row + u0) & 3) == 0;
            if (p.depth) {
                if (whole) {
                    float4_t zz = {z[0], z[1], z[2], z[3]};
                    *reinterpret_cast<float4_t*>(p.depth + row + u0) = zz;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (u0 + j >= 0 && u0 + j < p.W) p.depth[row + u0 + j] = z[j];
                }
            }
            if (p.mask) {
                if (whole) {
                    uchar4_t kk = {(unsigned char)(z[0] > 0.f), (unsigned char)(z[1] > 0.f), (unsigned char)(z[2] > 0.f), (unsigned char)(z[3] > 0.f)};
                    *reinterpret_cast<uchar4_t*>(p.mask + row + u0) = kk;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (u0 + j >= 0 && u0 + j < p.W) p.mask[row + u0 + j] = (unsigned char)(z[j] > 0.f);
                }
            }
        }
    }
    if (p.tile_counts) {
        n = block_sum_int(n, red);
        if (threadIdx.x == 0) p.tile_counts[(size_t)b * p.tiles + tile] = n;
    }
}

template <bool VEC, typename IT>
__global__ __launch_bounds__(kCloudThreads) void cloud_scatter_kernel(const CloudParams p) {
    __shared__ int red[kCloudThreads / 64];
    __shared__ int wave_n[2][kCloudThreads / 64];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // kept pixels of this pair in the tiles before this one
    const int* counts = p.tile_counts + (size_t)b * p.tiles;
    int before = 0;
    for (int t = threadIdx.x; t < tile; t += kCloudThreads) before += counts[t];
    long long base = block_sum_int(before, red);

    const IT* img = static_cast<const IT*>(p.image) + (size_t)b * 3 * p.H * p.W;
    const size_t plane = (size_t)p.H * p.W;
    uint4_t* rec = p.records + (size_t)b * (size_t)p.capacity;
    const int shift = p.ox & 3;
    const int v_end = min(p.H, (tile + 1) * p.rows_per_tile);
    int step = 0;
    for (int v = tile * p.rows_per_tile; v < v_end; ++v) {
        for (int c0 = -shift; c0 < p.W; c0 += kCloudChunk, ++step) {       // block-uniform: every wave takes every step (barrier inside)
            const int u0 = c0 + (int)threadIdx.x * 4;
            float z[4] = {0.f, 0.f, 0.f, 0.f};
            if (u0 < p.W) cloud_eval4<VEC>(p, b, v, u0, z);
            // rank inside the wave: the pixels of the lanes below come first, then this lane's own earlier pixels
            int below = 0, wave_total = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned long long bal = __ballot(z[j] > 0.f);
                below += __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
                wave_total += __popcll(bal);
            }
            if (lane == 0) wave_n[step & 1][wave] = wave_total;
            __syncthreads();                             // (two buffers: the step after next rewrites this one behind the next barrier)
            long long r = base;
            int block_total = 0;
#pragma unroll
            for (int w = 0; w < kCloudThreads / 64; ++w) {
                const int nw = wave_n[step & 1][w];
                if (w < wave) r += nw;
                block_total += nw;
            }
            base += block_total;
            r += below;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (z[j] > 0.f) {
                    if (r < p.capacity) rec[r] = cloud_record<IT>(p, img, plane, v, u0 + j, z[j]);
                    ++r;
                }
            }
        }
    }
    if (tile == p.tiles - 1 && threadIdx.x == 0) p.count[b] = (int)base;
}

// every check of a s2m2_cloud_desc that include/s2m2_hip.h lists, then the kernel parameters: shared with s2m2_mesh (mesh.hip), which takes the
// same descriptor fields (`what` prefixes the messages)
int cloud_validate(const s2m2_cloud_desc* d, const char* what, CloudParams& p, bool& vec) {
    S2M2_REQUIRE(d->disp && d->occ && d->conf, "%s: null pointer (disp / occ / conf)", what);
    S2M2_REQUIRE(d->depth || d->mask || d->count, "%s: no output requested (depth, mask and count are all null pointers)", what);
    S2M2_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->Hp > 0 && d->Wp > 0, "%s: non-positive extents B=%d H=%d W=%d Hp=%d Wp=%d", what, d->B,
                 d->H, d->W, d->Hp, d->Wp);
    S2M2_REQUIRE(d->H <= d->Hp && d->W <= d->Wp, "%s: the image (H=%d, W=%d) is larger than the maps (Hp=%d, Wp=%d)", what, d->H, d->W, d->Hp,
                 d->Wp);
    S2M2_REQUIRE(cloud_extents_ok(d->B, d->H, d->W) && (long long)d->Hp * d->Wp < (1LL << 31), "%s: extents too large (B <= 65535, H*W < 2^31)",
                 what);
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
    p.rows_per_tile = cloud_tile_rows(d->W);
    p.tiles = (d->H + p.rows_per_tile - 1) / p.rows_per_tile;
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

static int cloud_impl(const s2m2_cloud_desc* d, void* stream) {
    S2M2_REQUIRE(d != nullptr, "cloud: null descriptor");
    S2M2_REQUIRE(!plan_recording(), "cloud: s2m2_cloud is not recorded in launch plans -- call it after s2m2_plan_end, behind s2m2_plan_run / "
                                    "s2m2_engine_run on the same stream");
    CloudParams p;
    bool vec = false;
    if (int rc = cloud_validate(d, "cloud", p, vec)) return rc;
    const dim3 grid(p.tiles, d->B), block(kCloudThreads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = vec ? launch<cloud_count_kernel<true>>("cloud (count)", grid, block, 0, s, p) : launch<cloud_count_kernel<false>>("cloud (count)", grid, block, 0, s, p))
        return rc;
    if (!d->count) return 0;
    return by_image_dtype(d->image_dtype, "cloud", [&](auto ti) {            // (validated above)
        using IT = decltype(ti);
        if (vec) return launch<cloud_scatter_kernel<true, IT>>("cloud (scatter)", grid, block, 0, s, p);
        return launch<cloud_scatter_kernel<false, IT>>("cloud (scatter)", grid, block, 0, s, p);
    });
}

}  // namespace s2m2

extern "C" size_t s2m2_cloud_workspace_bytes(int B, int H, int W) {
    if (!s2m2::cloud_extents_ok(B, H, W)) return 0;
    const int rows = s2m2::cloud_tile_rows(W);
    const size_t tiles = (size_t)B * ((H + rows - 1) / rows);
    return (tiles * sizeof(int) + 255) / 256 * 256;
}

extern "C" int s2m2_cloud(const s2m2_cloud_desc* desc, void* stream) { return s2m2::cloud_impl(desc, stream); }
