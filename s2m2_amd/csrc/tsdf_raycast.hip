// K26: K24's TSDF volume ray-cast into the depth, gradient and colour maps of a camera (include/s2m2_hip.h: s2m2_tsdf_raycast).
//   tsdf_raycast_kernel      one thread owns a target pixel and marches its ray through the samples z_k = z_near + k * step; a wave is an 8 x 8
//                            patch of pixels (a block 32 x 8), so that its rays walk neighbouring voxels and share cache lines.  A sample reads
//                            the first 8 bytes of the eight voxels around it (tsdf_tw); the 16-byte record is read once, at the hit, for the
//                            colour.  The loop runs over the part of [0, n_steps) that a slab clip of the ray against the grid box (with a
//                            margin above every rounding error of the sample positions) cannot prove to be outside the grid: the samples it
//                            leaves out are unobserved by the rule, in front of the first one have_prev is false and behind the last one no
//                            crossing can follow, so the result is the same bits.  A wave leaves the loop when all its lanes have.
// The covered pixels of a tile are summed in the block and added to count[b] with one atomic per tile: integer adds, order-independent.
#include "tsdf_device.h"

namespace s2m2 {

constexpr int kRaycastTileW = 32, kRaycastTileH = 8;     // pixels of a block: four waves of 8 x 8 side by side
constexpr int kRaycastMaxSteps = 65536;
constexpr unsigned kRaycastMaxBlocks = 1u << 22;          // tiles beyond are walked in grid strides
static_assert(kRaycastTileW * kRaycastTileH == kRasterThreads && kRaycastTileW == 8 * kRasterWaves, "a wave is an 8 x 8 patch");

struct TsdfRaycastParams {
    const uint4_t* volume;
    const float* poses;         // (B, 12) on the device
    float* depth;
    float* gradients;
    unsigned char* image;
    int* count;
    int B, Ht, Wt, tiles_x, tiles_y;
    unsigned tiles;             // B * tiles_y * tiles_x
    int Nx, Ny, Nz;
    int min_weight, n_steps;
    float fx, fy, cx, cy;
    float gx, gy, gz, vs;
    float z_near, step;
};

// the cell of a position g in voxel units: false unless the sample can be OBSERVED by its position (float comparisons before any conversion
// to int: a NaN or Inf fails them and no address is formed); lin = the cell's corner (0,0,0), fr = g - floorf(g)
__device__ __forceinline__ bool raycast_cell(const TsdfRaycastParams& p, const float (&g)[3], int& lin, float (&fr)[3]) {
#pragma clang fp contract(off)
    const float f0x = floorf(g[0]), f0y = floorf(g[1]), f0z = floorf(g[2]);
    if (!(f0x >= 0.f && f0x <= (float)(p.Nx - 2) && f0y >= 0.f && f0y <= (float)(p.Ny - 2) && f0z >= 0.f && f0z <= (float)(p.Nz - 2))) return false;
    lin = ((int)f0z * p.Ny + (int)f0y) * p.Nx + (int)f0x;
    fr[0] = g[0] - f0x; fr[1] = g[1] - f0y; fr[2] = g[2] - f0z;
    return true;
}

// the tsdf of the eight corners of the cell at lin, t[dx + 2 dy + 4 dz]: false unless all eight are observed
__device__ __forceinline__ bool raycast_corners(const TsdfRaycastParams& p, int lin, float (&t)[8]) {
    TsdfExtractParams x;
    x.volume = p.volume;
    const int sy = p.Nx, sz = p.Nx * p.Ny;
    int wmin = 0x7fffffff;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int w;
        tsdf_tw(x, lin + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz, t[c], w);
        wmin = min(wmin, w);
    }
    return wmin >= p.min_weight;
}

__device__ __forceinline__ float raycast_lerp(float lo, float hi, float fr) {
#pragma clang fp contract(off)
    const float d = hi - lo;
    const float m = fr * d;
    return lo + m;
}

// along x, then y, then z
__device__ __forceinline__ float raycast_value(const float (&t)[8], const float (&fr)[3]) {
    const float c00 = raycast_lerp(t[0], t[1], fr[0]), c10 = raycast_lerp(t[2], t[3], fr[0]);
    const float c01 = raycast_lerp(t[4], t[5], fr[0]), c11 = raycast_lerp(t[6], t[7], fr[0]);
    return raycast_lerp(raycast_lerp(c00, c10, fr[1]), raycast_lerp(c01, c11, fr[1]), fr[2]);
}

// [lo, hi] := [lo, hi] intersected with the z at which a + z * b lies in [-m, n + m]; b == 0: all or nothing
__device__ __forceinline__ void raycast_slab(float a, float b, float n, float m, float& lo, float& hi) {
#pragma clang fp contract(off)
    if (b == 0.f) {
        if (!(a >= -m && a <= n + m)) hi = -INFINITY;
        return;
    }
    const float z0 = (-m - a) / b, z1 = ((n + m) - a) / b;        // finite numerators over a finite b != 0: never NaN
    lo = fmaxf(lo, fminf(z0, z1));
    hi = fminf(hi, fmaxf(z0, z1));
}

__global__ __launch_bounds__(kRasterThreads) void tsdf_raycast_kernel(const TsdfRaycastParams p) {
#pragma clang fp contract(off)
    __shared__ int red[kRasterWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px = wave * 8 + (lane & 7), py = lane >> 3;
    const size_t plane = (size_t)p.Ht * p.Wt;
    for (unsigned tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {      // block-uniform (tiles + gridDim.x < 2^32)
        const unsigned row = tile / (unsigned)p.tiles_x;
        const int tx = (int)(tile - row * (unsigned)p.tiles_x);
        const int b = (int)(row / (unsigned)p.tiles_y);
        const int ty = (int)row - b * p.tiles_y;
        const int u = tx * kRaycastTileW + px, v = ty * kRaycastTileH + py;
        const bool inside = u < p.Wt && v < p.Ht;
        const float* q = p.poses + (size_t)b * 12;

        // the ray in voxel units: g = a + z * b
        const float dx = ((float)u - p.cx) / p.fx, dy = ((float)v - p.cy) / p.fy;
        const float tx_ = q[3], ty_ = q[7], tz_ = q[11];
        const float org[3] = {p.gx, p.gy, p.gz};
        float ra[3], rb[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float w = (q[a] * dx + q[4 + a] * dy) + q[8 + a];
            const float o = -((q[a] * tx_ + q[4 + a] * ty_) + q[8 + a] * tz_);
            ra[a] = (o - org[a]) / p.vs;
            rb[a] = w / p.vs;
        }

        // the samples that may be observed: k0 <= k < k1.  A computed position differs from a + z b by less than 2^-22 (|a| + |z b|), and z_k
        // from z_near + k step by less than 2^-22 |z_k|; the margins are several times that, plus a voxel and two steps.
        int k0 = 0, k1 = 0;
        const float z_last = p.z_near + (float)p.n_steps * p.step;
        const bool finite = fabsf(ra[0]) < INFINITY && fabsf(ra[1]) < INFINITY && fabsf(ra[2]) < INFINITY && fabsf(rb[0]) < INFINITY &&
                            fabsf(rb[1]) < INFINITY && fabsf(rb[2]) < INFINITY;
        if (inside && finite) {                                               // a non-finite ray has no observed sample
            float lo = p.z_near, hi = z_last;
            const float ext[3] = {(float)(p.Nx - 1), (float)(p.Ny - 1), (float)(p.Nz - 1)};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float m = 1.0f + 4e-6f * ((fabsf(ra[a]) + z_last * fabsf(rb[a])) + ext[a]);
                raycast_slab(ra[a], rb[a], ext[a], m, lo, hi);
            }
            const float zm = 2.0f * p.step + 4e-6f * z_last;
            lo = lo - zm; hi = hi + zm;
            if (!(z_last < INFINITY)) {                                       // no clip where its own arithmetic would overflow
                k1 = p.n_steps;
            } else if (lo <= hi) {                                            // false also for a NaN
                const float f0 = floorf((lo - p.z_near) / p.step) - 1.0f, f1 = ceilf((hi - p.z_near) / p.step) + 2.0f;
                k0 = (int)fminf(fmaxf(f0, 0.f), (float)p.n_steps);
                k1 = (int)fminf(fmaxf(f1, 0.f), (float)p.n_steps);
            }
        }

        // the march
        bool have_prev = false, crossed = false;
        float t_prev = 0.f, z_prev = 0.f, t_hit = 0.f, z_k = 0.f;
        for (int k = k0; k < k1; ++k) {
            z_k = p.z_near + (float)k * p.step;
            const float g[3] = {ra[0] + z_k * rb[0], ra[1] + z_k * rb[1], ra[2] + z_k * rb[2]};
            int lin;
            float fr[3], t[8];
            if (!raycast_cell(p, g, lin, fr) || !raycast_corners(p, lin, t)) {
                have_prev = false;
                continue;
            }
            const float tv = raycast_value(t, fr);
            if (have_prev && !(t_prev < 0.f) && tv < 0.f) {
                crossed = true;
                t_hit = tv;
                break;
            }
            have_prev = true; t_prev = tv; z_prev = z_k;
        }

        // the hit
        float depth = 0.f, G[3] = {0.f, 0.f, 0.f};
        unsigned rgb[3] = {0u, 0u, 0u};
        bool covered = false;
        if (crossed) {
            const float z_hit = z_prev + (t_prev / (t_prev - t_hit)) * (z_k - z_prev);
            const float g[3] = {ra[0] + z_hit * rb[0], ra[1] + z_hit * rb[1], ra[2] + z_hit * rb[2]};
            int lin;
            float fr[3], t[8];
            if (raycast_cell(p, g, lin, fr) && raycast_corners(p, lin, t)) {
                covered = true;
                depth = z_hit;
                if (p.gradients) {
                    G[0] = raycast_lerp(raycast_lerp(t[1] - t[0], t[3] - t[2], fr[1]), raycast_lerp(t[5] - t[4], t[7] - t[6], fr[1]), fr[2]);
                    G[1] = raycast_lerp(raycast_lerp(t[2] - t[0], t[3] - t[1], fr[0]), raycast_lerp(t[6] - t[4], t[7] - t[5], fr[0]), fr[2]);
                    G[2] = raycast_lerp(raycast_lerp(t[4] - t[0], t[5] - t[1], fr[0]), raycast_lerp(t[6] - t[2], t[7] - t[3], fr[0]), fr[1]);
                }
                if (p.image) {
                    const int sel = lin + (fr[0] >= 0.5f ? 1 : 0) + (fr[1] >= 0.5f ? p.Nx : 0) + (fr[2] >= 0.5f ? p.Nx * p.Ny : 0);
                    const uint4_t o = *(const __attribute__((address_space(1))) uint4_t*)(p.volume + sel);
                    rgb[0] = ((o[2] & 0xffffu) + 128u) >> 8; rgb[1] = ((o[2] >> 16) + 128u) >> 8; rgb[2] = ((o[3] & 0xffffu) + 128u) >> 8;
                }
            }
        }

        if (inside) {
            const size_t pix = (size_t)v * p.Wt + u;
            if (p.depth) p.depth[(size_t)b * plane + pix] = depth;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                if (p.gradients) p.gradients[((size_t)b * 3 + ch) * plane + pix] = G[ch];
                if (p.image) p.image[((size_t)b * 3 + ch) * plane + pix] = (unsigned char)rgb[ch];
            }
        }
        if (p.count) {
            const int n = block_sum_int(covered ? 1 : 0, red);
            if (threadIdx.x == 0 && n) atomicAdd(p.count + b, n);
            __syncthreads();                                                  // red is written again by the next tile
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host

static int tsdf_raycast_impl(const s2m2_tsdf_raycast_desc* d, void* stream) {
    S2M2_REQUIRE(d != nullptr, "tsdf_raycast: null descriptor");
    if (int rc = refuse_while_recording("tsdf_raycast")) return rc;
    if (int rc = tsdf_check_volume("tsdf_raycast", d->volume, d->Nx, d->Ny, d->Nz, d->origin, d->voxel_size)) return rc;
    S2M2_REQUIRE(d->poses != nullptr, "tsdf_raycast: null pointer (poses)");
    S2M2_REQUIRE(((uintptr_t)d->poses & 3) == 0, "tsdf_raycast: poses must be 4-byte aligned");
    S2M2_REQUIRE(d->depth || d->gradients || d->image || d->count,
                 "tsdf_raycast: no output requested (depth, gradients, image and count are all null pointers)");
    S2M2_REQUIRE((((uintptr_t)d->depth | (uintptr_t)d->gradients | (uintptr_t)d->count) & 3) == 0,
                 "tsdf_raycast: depth, gradients and count must be 4-byte aligned");
    S2M2_REQUIRE(d->B > 0 && d->Ht > 0 && d->Wt > 0, "tsdf_raycast: non-positive extents B=%d Ht=%d Wt=%d", d->B, d->Ht, d->Wt);
    S2M2_REQUIRE((long long)d->Ht * d->Wt < (1LL << 31) && (long long)d->B * ((long long)d->Ht * d->Wt) < (1LL << 31),
                 "tsdf_raycast: extents too large (B*Ht*Wt < 2^31)");
    S2M2_REQUIRE(tsdf_finite_f32(d->fx) && tsdf_finite_f32(d->fy) && (float)d->fx != 0.f && (float)d->fy != 0.f,
                 "tsdf_raycast: fx and fy must be finite and non-zero in fp32 (fx=%g fy=%g)", d->fx, d->fy);
    S2M2_REQUIRE(tsdf_finite_f32(d->cx) && tsdf_finite_f32(d->cy), "tsdf_raycast: cx and cy must be finite (also in fp32)");
    S2M2_REQUIRE(d->min_weight >= 1, "tsdf_raycast: min_weight must be >= 1 (%d)", d->min_weight);
    S2M2_REQUIRE(tsdf_finite_f32(d->z_near) && tsdf_finite_f32(d->z_far) && tsdf_finite_f32(d->step),
                 "tsdf_raycast: z_near, z_far and step must be finite (also in fp32)");
    const float z_near = (float)d->z_near, z_far = (float)d->z_far, step = (float)d->step;
    S2M2_REQUIRE(z_near >= 0.f && z_near < z_far && step > 0.f,
                 "tsdf_raycast: 0 <= z_near < z_far and step > 0 are required in fp32 (z_near=%g z_far=%g step=%g)", d->z_near, d->z_far, d->step);
    const double n_steps = ceil(((double)z_far - (double)z_near) / (double)step);
    S2M2_REQUIRE(n_steps <= (double)kRaycastMaxSteps, "tsdf_raycast: %.0f steps from z_near to z_far (at most %d)", n_steps, kRaycastMaxSteps);

    TsdfRaycastParams p;
    p.volume = static_cast<const uint4_t*>(d->volume);
    p.poses = d->poses;
    p.depth = d->depth; p.gradients = d->gradients; p.image = d->image; p.count = d->count;
    p.B = d->B; p.Ht = d->Ht; p.Wt = d->Wt;
    p.tiles_x = (d->Wt + kRaycastTileW - 1) / kRaycastTileW;
    p.tiles_y = (d->Ht + kRaycastTileH - 1) / kRaycastTileH;
    p.tiles = (unsigned)((long long)d->B * p.tiles_y * p.tiles_x);               // <= B*Ht*Wt < 2^31
    p.Nx = d->Nx; p.Ny = d->Ny; p.Nz = d->Nz;
    p.min_weight = d->min_weight;
    p.n_steps = (int)n_steps;
    p.fx = (float)d->fx; p.fy = (float)d->fy; p.cx = (float)d->cx; p.cy = (float)d->cy;
    p.gx = (float)d->origin[0]; p.gy = (float)d->origin[1]; p.gz = (float)d->origin[2];
    p.vs = (float)d->voxel_size;
    p.z_near = z_near; p.step = step;

    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d->count && hipMemsetAsync(d->count, 0, sizeof(int) * (size_t)d->B, s) != hipSuccess) return set_error("tsdf_raycast: memset failed");
    const dim3 grid(p.tiles < kRaycastMaxBlocks ? p.tiles : kRaycastMaxBlocks), block(kRasterThreads);
    return launch<tsdf_raycast_kernel>("tsdf_raycast", grid, block, 0, s, p);
}

}  // namespace s2m2

extern "C" int s2m2_tsdf_raycast(const s2m2_tsdf_raycast_desc* desc, void* stream) { return s2m2::tsdf_raycast_impl(desc, stream); }
