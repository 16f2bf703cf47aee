// K15: the 3D output stage behind the forward (include/s2m2_hip.h: s2m2_cloud) -- validity filter, metric depth, and the kept pixels compacted
// into a coloured point cloud in raster order.  Two launches without a host step, atomics or waiting between blocks:
//   cloud_count_kernel    a block owns a tile of whole image rows: dense depth / mask, one count per tile into the workspace
//   cloud_scatter_kernel  a block sums the counts of the tiles before its own (strided over the block, wave + block reduction), recomputes
//                         keep, ranks its pixels (wave ballots + mbcnt, a prefix over the four waves through LDS) and stores the records
// Pixel -> thread map: a thread owns four consecutive pixels of one row, placed so that their MAP column is a multiple of four whatever the crop
// offset is (the first group of a row starts (Wp-W)/2 % 4 pixels left of the image): with Wp % 4 == 0 every map read is one aligned 16-byte
// load that stays inside the padded row.  Image reads and the dense stores follow the unpadded rows and are per pixel unless a group is aligned.
#include "common.h"
#include "launch.h"
#include "plan.h"

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

// the four pixels of this thread in image row v, first column u0 (may be < 0 or reach beyond W: those pixels give z = 0)
template <bool VEC>
__device__ __forceinline__ void cloud_eval4(const CloudParams& p, int b, int v, int u0, float z[4]) {
    const size_t m = ((size_t)b * p.Hp + (v + p.oy)) * (size_t)p.Wp + (size_t)(p.ox + u0);      // p.ox + u0 >= 0 by construction
    float d[4], o[4], c[4];
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

__device__ __forceinline__ int wave_sum_int(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// sum over the block of one int per thread, result in every thread (red: kCloudThreads / 64 ints of LDS)
__device__ __forceinline__ int block_sum_int(int x, int* red) {
    x = wave_sum_int(x);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < kCloudThreads / 64; ++w) s += red[w];
    return s;
}

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

template <typename IT> __device__ __forceinline__ unsigned cloud_byte(IT x);
template <> __device__ __forceinline__ unsigned cloud_byte<unsigned char>(unsigned char x) { return x; }
template <> __device__ __forceinline__ unsigned cloud_byte<float>(float x) { return (unsigned)__float2int_rn(fminf(fmaxf(x, 0.f), 255.f)); }
template <> __device__ __forceinline__ unsigned cloud_byte<half_t>(half_t x) { return cloud_byte<float>((float)x); }

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
        const size_t row = (size_t)v * p.W;
        const float fv = (float)v - p.cy;
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
                    if (r < p.capacity) {
                        const int u = u0 + j;
                        const size_t px = row + u;
                        const unsigned cr = cloud_byte<IT>(img[px]), cg = cloud_byte<IT>(img[plane + px]), cb = cloud_byte<IT>(img[2 * plane + px]);
                        const float x = ((float)u - p.cx) * z[j] / p.fx;
                        const float y = fv * z[j] / p.fy;
                        uint4_t o = {__builtin_bit_cast(unsigned, x), __builtin_bit_cast(unsigned, y), __builtin_bit_cast(unsigned, z[j]),
                                     cr | (cg << 8) | (cb << 16) | 0xff000000u};
                        rec[r] = o;
                    }
                    ++r;
                }
            }
        }
    }
    if (tile == p.tiles - 1 && threadIdx.x == 0) p.count[b] = (int)base;
}

static bool cloud_extents_ok(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 31) && B <= 65535;
}

static int cloud_impl(const s2m2_cloud_desc* d, void* stream) {
    S2M2_REQUIRE(d != nullptr, "cloud: null descriptor");
    S2M2_REQUIRE(!plan_recording(), "cloud: s2m2_cloud is not recorded in launch plans -- call it after s2m2_plan_end, behind s2m2_plan_run / "
                                    "s2m2_engine_run on the same stream");
    S2M2_REQUIRE(d->disp && d->occ && d->conf, "cloud: null pointer (disp / occ / conf)");
    S2M2_REQUIRE(d->depth || d->mask || d->count, "cloud: no output requested (depth, mask and count are all null pointers)");
    S2M2_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->Hp > 0 && d->Wp > 0, "cloud: non-positive extents B=%d H=%d W=%d Hp=%d Wp=%d", d->B, d->H,
                 d->W, d->Hp, d->Wp);
    S2M2_REQUIRE(d->H <= d->Hp && d->W <= d->Wp, "cloud: the image (H=%d, W=%d) is larger than the maps (Hp=%d, Wp=%d)", d->H, d->W, d->Hp, d->Wp);
    S2M2_REQUIRE(cloud_extents_ok(d->B, d->H, d->W) && (long long)d->Hp * d->Wp < (1LL << 31), "cloud: extents too large (B <= 65535, H*W < 2^31)");
    S2M2_REQUIRE(d->fx > 0.0 && d->fy > 0.0, "cloud: fx and fy must be positive (fx=%g fy=%g)", d->fx, d->fy);
    S2M2_REQUIRE(d->depth_scale > 0.0, "cloud: depth_scale must be positive (%g)", d->depth_scale);
    S2M2_REQUIRE(d->capacity >= 0, "cloud: negative capacity %lld", d->capacity);
    S2M2_REQUIRE(d->image_dtype == S2M2_F32 || d->image_dtype == S2M2_F16 || d->image_dtype == 2, "cloud: unsupported image dtype %d", d->image_dtype);
    if (d->count) {
        S2M2_REQUIRE(d->image != nullptr, "cloud: null pointer (image) while a cloud is requested");
        S2M2_REQUIRE(d->workspace != nullptr, "cloud: null workspace while a cloud is requested (s2m2_cloud_workspace_bytes)");
        S2M2_REQUIRE(((uintptr_t)d->workspace & 3) == 0, "cloud: the workspace must be 4-byte aligned");
        S2M2_REQUIRE(d->records != nullptr || d->capacity == 0, "cloud: null pointer (records) with capacity %lld", d->capacity);
        S2M2_REQUIRE(((uintptr_t)d->records & 15) == 0, "cloud: records must be 16-byte aligned");
    }
    S2M2_REQUIRE(((uintptr_t)d->depth & 3) == 0 && ((uintptr_t)d->disp & 3) == 0 && ((uintptr_t)d->occ & 3) == 0 && ((uintptr_t)d->conf & 3) == 0,
                 "cloud: fp32 tensors must be 4-byte aligned");

    CloudParams p;
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
    S2M2_REQUIRE(p.fx > 0.f && p.fy > 0.f && p.depth_scale > 0.f, "cloud: fx, fy and depth_scale must be positive in fp32");
    // the aligned form: 16-byte map loads.  The dense outputs take 16-byte / 4-byte group stores only where their own address allows it
    // (checked per group in the kernel against the element index: that needs the base pointers aligned too, else the per-pixel form)
    const bool vec = d->Wp % 4 == 0 && (((uintptr_t)d->disp | (uintptr_t)d->occ | (uintptr_t)d->conf) & 15) == 0 &&
                     ((uintptr_t)d->depth & 15) == 0 && ((uintptr_t)d->mask & 3) == 0;
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
