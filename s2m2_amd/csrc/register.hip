// K21: the depth map registered to a second camera (include/s2m2_hip.h: s2m2_register) -- a z-buffered forward warp of the kept pixels of the
// left view into a target camera.  Three launches without a host step:
//   register_clear_kernel    the z-buffer (one 64-bit key per target pixel, in the workspace) to all ones, count and visible to 0
//   register_splat_kernel    K15's tile walk and map loads (raster_tiles.h, cloud_device.h: cloud_eval4); every kept pixel is back-projected,
//                            transformed, projected (register_project) and its key is folded into the footprint's target pixels with a 64-bit
//                            atomic minimum whose value is not used.  A thread's four pixels are consecutive in a row, so the atomics of a wave
//                            fall on mostly contiguous 8-byte words of a target row; the z change lanes inside the wave first, so that
//                            the lanes of one atomic instruction hold neighbouring pixels (S2M2_REGISTER_LANE_ORDER below).
//   register_resolve_kernel  a thread takes four consecutive target pixels of one pair: decodes the keys, stores depth_t / index_t / image_t
//                            (dense_store4), marks the winners in visible and adds the block's covered pixels to count[b] with one atomic add
// The minimum of unique keys and an integer sum do not depend on the order of arrival: the outputs are bit-reproducible.
#include "cloud_device.h"
#include "launch.h"
#include "plan.h"

#include <math.h>

namespace s2m2 {

constexpr unsigned long long kRegisterEmpty = ~0ull;     // a cleared target pixel

struct RegisterParams {
    CloudParams c;              // the inputs and the tile geometry of K15 (its outputs are null)
    unsigned long long* zbuf;   // (B, Ht, Wt) keys
    float* depth_t;
    int* index_t;
    unsigned char* image_t;
    unsigned char* visible;
    int* count;
    int Ht, Wt, splat;
    float fx_t, fy_t, cx_t, cy_t;
    float r[9], t[3];
    float centre;               // (splat - 2) / 2
    int vec_f32, vec_i32, vec_u8;   // depth_t / index_t 16-byte aligned, image_t 4-byte aligned: dense_store4 may move a group whole
};

// ---------------------------------------------------------------------------------------------------------------- (A) clear

// n bytes at p to the byte v, over the whole grid: 16-byte stores between the first and the last 16-byte boundary, bytes outside
__device__ __forceinline__ void register_fill(unsigned char* p, size_t n, unsigned char v) {
    if (!p || n == 0) return;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (size_t)gridDim.x * blockDim.x;
    size_t head = (size_t)(-(uintptr_t)p & 15);
    if (head > n) head = n;
    const size_t body = (n - head) / 16, tail = n - head - body * 16;
    const unsigned w = v * 0x01010101u;
    const uint4_t vv = {w, w, w, w};
    uint4_t* q = reinterpret_cast<uint4_t*>(p + head);
    for (size_t i = tid; i < body; i += nthreads) q[i] = vv;
    if (tid < head) p[tid] = v;
    if (tid < tail) p[head + body * 16 + tid] = v;
}

__global__ __launch_bounds__(kRasterThreads) void register_clear_kernel(const RegisterParams p, size_t zbuf_bytes, size_t visible_bytes, size_t count_bytes) {
    register_fill(reinterpret_cast<unsigned char*>(p.zbuf), zbuf_bytes, 0xff);
    register_fill(p.visible, visible_bytes, 0);
    register_fill(reinterpret_cast<unsigned char*>(p.count), count_bytes, 0);
}

// ---------------------------------------------------------------------------------------------------------------- (B) splat

// The chain of the header from the kept pixel (v, u) with depth z to the footprint origin: false = nothing lands.  One IEEE rounding per
// operation; the library is compiled with -ffp-contract=on, so contraction is switched off for this block.
__device__ __forceinline__ bool register_project(const RegisterParams& p, int v, int u, float z, float& Z, int& fu, int& fv) {
#pragma clang fp contract(off)
    const CloudParams& c = p.c;
    const float x = ((float)u - c.cx) * z / c.fx;
    const float y = ((float)v - c.cy) * z / c.fy;
    const float X = ((p.r[0] * x + p.r[1] * y) + p.r[2] * z) + p.t[0];
    const float Y = ((p.r[3] * x + p.r[4] * y) + p.r[5] * z) + p.t[1];
    Z = ((p.r[6] * x + p.r[7] * y) + p.r[8] * z) + p.t[2];
    if (!(Z > 0.f && Z < INFINITY)) return false;
    const float up = (p.fx_t * X) / Z + p.cx_t;
    const float vp = (p.fy_t * Y) / Z + p.cy_t;
    const float ffu = floorf(up - p.centre), ffv = floorf(vp - p.centre);
    const float lo = -(float)p.splat;
    if (!(ffu >= lo && ffu < (float)p.Wt && ffv >= lo && ffv < (float)p.Ht)) return false;      // a NaN fails; both now fit an int
    fu = (int)ffu;
    fv = (int)ffv;
    return true;
}

// One kept pixel: project it and fold its key into the footprint's target pixels
template <int SPLAT>
__device__ __forceinline__ void register_splat_pixel(const RegisterParams& p, unsigned long long* zb, int v, int u, float z) {
    float Z;
    int fu, fv;
    if (!register_project(p, v, u, z, Z, fu, fv)) return;
    const unsigned long long key = ((unsigned long long)__builtin_bit_cast(unsigned, Z) << 32) | (unsigned)(v * p.c.W + u);
#pragma unroll
    for (int dy = 0; dy < SPLAT; ++dy) {
        const int tv = fv + dy;
        if (tv < 0 || tv >= p.Ht) continue;
#pragma unroll
        for (int dx = 0; dx < SPLAT; ++dx) {
            const int tu = fu + dx;
            if (tu >= 0 && tu < p.Wt) atomicMin(zb + (size_t)tv * p.Wt + tu, key);
        }
    }
}

// S2M2_REGISTER_LANE_ORDER (default 1): the z of a wave's 256 pixels change lanes through LDS behind the loads, so that lane l splats the
// pixels l, 64 + l, 128 + l, 192 + l of the wave's span: neighbouring lanes of ONE atomic instruction then hold neighbouring source pixels,
// whose footprints are neighbouring 8-byte words of a target row (one contiguous piece per instruction: the shape global atomics run
// fastest in), instead of every fourth.  0: a thread splats the four pixels it loaded (profiles/register/lane_order.txt has both).  The
// keys, and so the result, are the same either way.
#ifndef S2M2_REGISTER_LANE_ORDER
#define S2M2_REGISTER_LANE_ORDER 1
#endif

template <bool VEC, int SPLAT>
__global__ __launch_bounds__(kRasterThreads) void register_splat_kernel(const RegisterParams p) {
    const CloudParams& c = p.c;
    const int b = blockIdx.y, tile = blockIdx.x;
    unsigned long long* zb = p.zbuf + (size_t)b * p.Ht * p.Wt;
#if S2M2_REGISTER_LANE_ORDER
    __shared__ float zs[kRasterWaves][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#endif
    for (RasterWalk w(c, tile, c.H); w.more(); w.next()) {
        const int v = w.v, u0 = w.u0();
        float z[4] = {0.f, 0.f, 0.f, 0.f};              // 0: not kept (also the pixels of the group outside [0, W))
        if (u0 < c.W) cloud_eval4<VEC>(c, b, v, u0, z);
#if S2M2_REGISTER_LANE_ORDER
        __syncthreads();                                 // the reads of the step before are done (block-uniform walk: raster_tiles.h)
#pragma unroll
        for (int j = 0; j < 4; ++j) zs[wave][lane * 4 + j] = z[j];
        __syncthreads();
        const int uw = w.c0 + wave * 256;                // image column of the wave's first pixel
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float zz = zs[wave][j * 64 + lane];
            if (zz > 0.f) register_splat_pixel<SPLAT>(p, zb, v, uw + j * 64 + lane, zz);
        }
#else
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (z[j] > 0.f) register_splat_pixel<SPLAT>(p, zb, v, u0 + j, z[j]);
#endif
    }
}

// ---------------------------------------------------------------------------------------------------------------- (C) resolve

template <typename IT>
__global__ __launch_bounds__(kRasterThreads) void register_resolve_kernel(const RegisterParams p) {
    __shared__ int red[kRasterWaves];
    const CloudParams& c = p.c;
    const int b = blockIdx.y;
    const int n = p.Ht * p.Wt;                                                  // target pixels of one pair (< 2^31)
    const long long i0l = ((long long)blockIdx.x * kRasterThreads + threadIdx.x) * 4;
    const size_t base = (size_t)b * n;                                         // the pair's first target pixel
    const size_t plane = (size_t)c.H * c.W;
    int covered = 0;
    if (i0l < n) {
        const int i0 = (int)i0l;
        float depth[4];
        int index[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned long long key = i0 + j < n ? p.zbuf[base + i0 + j] : kRegisterEmpty;
            const bool hit = key != kRegisterEmpty;
            depth[j] = hit ? __builtin_bit_cast(float, (unsigned)(key >> 32)) : 0.f;
            index[j] = hit ? (int)(unsigned)key : -1;
            covered += hit;
        }
        if (p.depth_t) dense_store4(p.depth_t, base, i0, n, p.vec_f32 != 0, depth);
        if (p.index_t) dense_store4(p.index_t, base, i0, n, p.vec_i32 != 0, index);
        if (p.image_t) {
            const IT* img = static_cast<const IT*>(c.image) + (size_t)b * 3 * plane;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                unsigned char col[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) col[j] = index[j] >= 0 ? (unsigned char)cloud_byte<IT>(img[ch * plane + index[j]]) : (unsigned char)0;
                dense_store4(p.image_t, ((size_t)b * 3 + ch) * n, i0, n, p.vec_u8 != 0, col);
            }
        }
        if (p.visible) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (index[j] >= 0) p.visible[(size_t)b * plane + index[j]] = 1;
        }
    }
    if (p.count) {
        covered = block_sum_int(covered, red);
        if (threadIdx.x == 0 && covered) atomicAdd(p.count + b, covered);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host

static bool finite_f32(double x) { return isfinite(x) && isfinite((float)x); }

template <bool VEC>
static int register_splat(const RegisterParams& p, dim3 grid, hipStream_t s) {
    const dim3 block(kRasterThreads);
    switch (p.splat) {
        case 1: return launch<register_splat_kernel<VEC, 1>>("register (splat)", grid, block, 0, s, p);
        case 2: return launch<register_splat_kernel<VEC, 2>>("register (splat)", grid, block, 0, s, p);
        case 3: return launch<register_splat_kernel<VEC, 3>>("register (splat)", grid, block, 0, s, p);
        default: return launch<register_splat_kernel<VEC, 4>>("register (splat)", grid, block, 0, s, p);
    }
}

static int register_impl(const s2m2_register_desc* d, void* stream) {
    S2M2_REQUIRE(d != nullptr, "register: null descriptor");
    if (int rc = refuse_while_recording("register")) return rc;
    RegisterParams p;
    bool vec = false;
    s2m2_cloud_desc in = d->cloud;                  // the inputs alone: the output fields of the embedded descriptor are ignored
    in.depth = nullptr; in.mask = nullptr; in.records = nullptr; in.count = nullptr; in.workspace = nullptr; in.capacity = 0;
    if (int rc = cloud_validate(&in, "register", kCloudTilePixels, p.c, vec, false)) return rc;
    S2M2_REQUIRE(d->Ht > 0 && d->Wt > 0, "register: non-positive target extents Ht=%d Wt=%d", d->Ht, d->Wt);
    S2M2_REQUIRE((long long)d->Ht * d->Wt < (1LL << 31), "register: target extents too large (Ht*Wt < 2^31)");
    S2M2_REQUIRE(d->splat >= 1 && d->splat <= 4, "register: splat must be 1..4 (%d)", d->splat);
    bool finite = finite_f32(d->fx_t) && finite_f32(d->fy_t) && finite_f32(d->cx_t) && finite_f32(d->cy_t);
    for (int i = 0; i < 9; ++i) finite = finite && finite_f32(d->R[i]);
    for (int i = 0; i < 3; ++i) finite = finite && finite_f32(d->t[i]);
    S2M2_REQUIRE(finite, "register: R, t and the target intrinsics must be finite (also in fp32)");
    S2M2_REQUIRE(d->fx_t > 0.0 && d->fy_t > 0.0 && (float)d->fx_t > 0.f && (float)d->fy_t > 0.f,
                 "register: fx_t and fy_t must be positive (fx_t=%g fy_t=%g)", d->fx_t, d->fy_t);
    S2M2_REQUIRE(d->depth_t || d->index_t || d->image_t || d->visible || d->count,
                 "register: no output requested (depth_t, index_t, image_t, visible and count are all null pointers)");
    S2M2_REQUIRE(!d->image_t || d->cloud.image, "register: null pointer (cloud.image) while image_t is requested");
    S2M2_REQUIRE(d->workspace != nullptr, "register: null workspace (s2m2_register_workspace_bytes)");
    S2M2_REQUIRE(((uintptr_t)d->workspace & 7) == 0, "register: the workspace must be 8-byte aligned");
    S2M2_REQUIRE((((uintptr_t)d->depth_t | (uintptr_t)d->index_t | (uintptr_t)d->count) & 3) == 0,
                 "register: depth_t, index_t and count must be 4-byte aligned");

    p.zbuf = static_cast<unsigned long long*>(d->workspace);
    p.depth_t = d->depth_t; p.index_t = d->index_t; p.image_t = d->image_t; p.visible = d->visible; p.count = d->count;
    p.Ht = d->Ht; p.Wt = d->Wt; p.splat = d->splat;
    p.fx_t = (float)d->fx_t; p.fy_t = (float)d->fy_t; p.cx_t = (float)d->cx_t; p.cy_t = (float)d->cy_t;
    for (int i = 0; i < 9; ++i) p.r[i] = (float)d->R[i];
    for (int i = 0; i < 3; ++i) p.t[i] = (float)d->t[i];
    p.centre = (float)(d->splat - 2) * 0.5f;
    p.vec_f32 = ((uintptr_t)d->depth_t & 15) == 0;
    p.vec_i32 = ((uintptr_t)d->index_t & 15) == 0;
    p.vec_u8 = ((uintptr_t)d->image_t & 3) == 0;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 block(kRasterThreads);
    const size_t n = (size_t)d->Ht * d->Wt, B = (size_t)d->cloud.B;
    const size_t zbytes = B * n * sizeof(unsigned long long);
    const size_t clear_blocks = (zbytes / 16 + kRasterThreads - 1) / kRasterThreads;
    const dim3 clear_grid((unsigned)(clear_blocks < 1 ? 1 : clear_blocks > 4096 ? 4096 : clear_blocks));
    if (int rc = launch<register_clear_kernel>("register (clear)", clear_grid, block, 0, s, p, zbytes, B * (size_t)d->cloud.H * d->cloud.W, B * sizeof(int)))
        return rc;
    const dim3 grid(p.c.tiles, d->cloud.B);
    if (int rc = vec ? register_splat<true>(p, grid, s) : register_splat<false>(p, grid, s)) return rc;
    const dim3 rgrid((unsigned)((n + kRasterChunk - 1) / kRasterChunk), d->cloud.B);
    if (!d->image_t) return launch<register_resolve_kernel<unsigned char>>("register (resolve)", rgrid, block, 0, s, p);
    return by_image_dtype(d->cloud.image_dtype, "register", [&](auto ti) {
        using IT = decltype(ti);
        return launch<register_resolve_kernel<IT>>("register (resolve)", rgrid, block, 0, s, p);
    });
}

}  // namespace s2m2

extern "C" size_t s2m2_register_workspace_bytes(int B, int Ht, int Wt) {
    using namespace s2m2;
    if (!raster_extents_ok(B, Ht, Wt)) return 0;
    return round256((size_t)B * Ht * Wt * sizeof(unsigned long long));
}

extern "C" int s2m2_register(const s2m2_register_desc* desc, void* stream) { return s2m2::register_impl(desc, stream); }
