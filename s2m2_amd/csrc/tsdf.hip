// K24: depth maps of a moving rig fused into a truncated signed distance (TSDF) volume (include/s2m2_hip.h: s2m2_tsdf_integrate,
// s2m2_tsdf_extract) -- the first stage that carries state from one pair to the next.  The volume is caller-owned device memory, 16 bytes
// per voxel { float tsdf; int32 weight; uint16 r, g, b, pad }, voxel (i, j, k) at (k * Ny + j) * Nx + i; all zero = empty.
//   tsdf_integrate_kernel    one thread owns a voxel: the lanes of a wave are 64 neighbours in i, the four waves of a block four rows j, and a
//                            block walks the slices k in grid strides.  The loop over the B pairs of the call runs inside the thread: the voxel
//                            is read (one 16-byte load) when the first pair updates it and written (one 16-byte store) behind the last, and not
//                            touched at all when no pair does.  Per pair: K21's transform and projection with the pose from a DEVICE buffer
//                            (uniform loads), three gathered map reads, K15's keep / z (cloud_device.h: cloud_z), and the colour bytes only of
//                            a pixel that updates.  No atomics: bit-reproducible.
//   tsdf_count_kernel        a block owns a tile of kTsdfTileVoxels consecutive voxels and counts its surface points
//   tsdf_store_kernel        K15's scatter: tile_prefix, raster_rank_step with the three axis flags of a voxel, records and gradients
// A surface point is a sign change of the tsdf between an observed voxel and its observed +1 neighbour along x, y or z (tsdf_crossings), which
// both extraction launches evaluate alike.  The extraction's device functions and descriptor checks are in tsdf_device.h, which K25
// (tsdf_mesh.hip) shares.
#include "cloud_device.h"
#include "tsdf_device.h"

namespace s2m2 {

struct TsdfParams {
    CloudParams c;              // the inputs of K15 (its outputs are null)
    uint4_t* volume;
    const float* poses;         // (B, 12) on the device
    int B, Nx, Ny, Nz;
    int max_weight, carve;
    float gx, gy, gz, vs, trunc;    // centre of voxel (0,0,0), voxel size, truncation distance
};

// ---------------------------------------------------------------------------------------------------------------- integrate

// One IEEE rounding per operation: the library is compiled with -ffp-contract=on, so contraction is switched off for the kernel's body.
template <typename IT>
__global__ __launch_bounds__(kRasterThreads) void tsdf_integrate_kernel(const TsdfParams p) {
#pragma clang fp contract(off)
    const CloudParams& c = p.c;
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const size_t map_plane = (size_t)c.Hp * c.Wp, plane = (size_t)c.H * c.W;
    const size_t crop = (size_t)c.oy * c.Wp + c.ox;                  // image pixel (0, 0) in a padded map
    if (i >= p.Nx) return;
    const float x = p.gx + (float)i * p.vs;
    const float fW = (float)c.W, fH = (float)c.H;
    for (int j = blockIdx.y * kRasterWaves + (threadIdx.x >> 6); j < p.Ny; j += gridDim.y * kRasterWaves) {
        const float y = p.gy + (float)j * p.vs;
        for (int k = blockIdx.z; k < p.Nz; k += gridDim.z) {
            const float z = p.gz + (float)k * p.vs;
            uint4_t* vox = p.volume + ((size_t)(k * p.Ny + j) * p.Nx + i);           // k * Ny + j < 2^29
            bool touched = false;
            float tsdf = 0.f;
            unsigned weight = 0, cr = 0, cg = 0, cb = 0, pad = 0;
            const float *disp = c.disp + crop, *occ = c.occ + crop, *conf = c.conf + crop;
            const IT* img = static_cast<const IT*>(c.image);
            const float* q = p.poses;
            for (int b = 0; b < p.B; ++b, disp += map_plane, occ += map_plane, conf += map_plane, img += 3 * plane, q += 12) {
                const float X = ((q[0] * x + q[1] * y) + q[2] * z) + q[3];
                const float Y = ((q[4] * x + q[5] * y) + q[6] * z) + q[7];
                const float Z = ((q[8] * x + q[9] * y) + q[10] * z) + q[11];
                if (!(Z > 0.f && Z < INFINITY)) continue;
                const float up = (c.fx * X) / Z + c.cx;
                const float vp = (c.fy * Y) / Z + c.cy;
                const float fu = rintf(up), fv = rintf(vp);
                if (!(fu >= 0.f && fu < fW && fv >= 0.f && fv < fH)) continue;       // a NaN fails; both now fit an int
                const int u = (int)fu, v = (int)fv;
                const int m = v * c.Wp + u;                                         // Hp * Wp < 2^31
                const float zp = cloud_z(c, disp[m], occ[m], conf[m]);
                if (!(zp > 0.f)) continue;
                const float sdf = zp - Z;
                if (!(sdf >= -p.trunc)) continue;
                if (!p.carve && sdf > p.trunc) continue;
                const float d = fminf(sdf / p.trunc, 1.0f);
                if (!touched) {
                    const uint4_t o = *(const __attribute__((address_space(1))) uint4_t*)vox;
                    tsdf = __builtin_bit_cast(float, o[0]);
                    weight = o[1];
                    cr = o[2] & 0xffffu; cg = o[2] >> 16; cb = o[3] & 0xffffu; pad = o[3] >> 16;
                    touched = true;
                }
                unsigned br, bg, bb;
                cloud_colour<IT>(c, img, plane, v, u, br, bg, bb);
                const float Wf = (float)(int)weight;
                tsdf = (tsdf * Wf + d) / (Wf + 1.0f);
                const unsigned w1 = weight + 1u, half = w1 >> 1;
                cr = (cr * weight + (br << 8) + half) / w1;
                cg = (cg * weight + (bg << 8) + half) / w1;
                cb = (cb * weight + (bb << 8) + half) / w1;
                weight = (unsigned)min((int)w1, p.max_weight);
            }
            if (touched) {
                const uint4_t o = {__builtin_bit_cast(unsigned, tsdf), weight, (cr & 0xffffu) | (cg << 16), (cb & 0xffffu) | (pad << 16)};
                *vox = o;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- extract

__global__ __launch_bounds__(kRasterThreads) void tsdf_count_kernel(const TsdfExtractParams p) {
    __shared__ int red[kRasterWaves];
    const int tile = blockIdx.x;
    const int end = min(p.n, (tile + 1) * kTsdfTileVoxels);
    int n = 0;
    for (int lin = tile * kTsdfTileVoxels + threadIdx.x; lin < end; lin += kRasterThreads) n += tsdf_points_of(p, lin);
    n = block_sum_int(n, red);
    if (threadIdx.x == 0) p.tile_counts[tile] = n;
}

__global__ __launch_bounds__(kRasterThreads) void tsdf_store_kernel(const TsdfExtractParams p) {
    __shared__ int red[kRasterWaves];
    __shared__ int wave_n[2][kRasterWaves];
    tsdf_store_tile<false>(p, nullptr, red, wave_n);
}

// ---------------------------------------------------------------------------------------------------------------- host

static int tsdf_integrate_impl(const s2m2_tsdf_desc* d, void* stream) {
    S2M2_REQUIRE(d != nullptr, "tsdf_integrate: null descriptor");
    if (int rc = refuse_while_recording("tsdf_integrate")) return rc;
    TsdfParams p;
    bool vec = false;
    s2m2_cloud_desc in = d->cloud;                  // the inputs alone: the output fields of the embedded descriptor are ignored
    in.depth = nullptr; in.mask = nullptr; in.records = nullptr; in.count = nullptr; in.workspace = nullptr; in.capacity = 0;
    if (int rc = cloud_validate(&in, "tsdf_integrate", kCloudTilePixels, p.c, vec, false)) return rc;
    S2M2_REQUIRE(d->cloud.image != nullptr, "tsdf_integrate: null pointer (image)");
    if (int rc = tsdf_check_volume("tsdf_integrate", d->volume, d->Nx, d->Ny, d->Nz, d->origin, d->voxel_size)) return rc;
    S2M2_REQUIRE(tsdf_positive_f32(d->trunc), "tsdf_integrate: trunc must be finite and > 0 in fp32 (%g)", d->trunc);
    S2M2_REQUIRE(d->max_weight >= 1 && d->max_weight <= 32767, "tsdf_integrate: max_weight must be 1..32767 (%d)", d->max_weight);
    S2M2_REQUIRE(d->poses != nullptr, "tsdf_integrate: null pointer (poses)");
    S2M2_REQUIRE(((uintptr_t)d->poses & 3) == 0, "tsdf_integrate: poses must be 4-byte aligned");

    p.volume = static_cast<uint4_t*>(d->volume);
    p.poses = d->poses;
    p.B = d->cloud.B; p.Nx = d->Nx; p.Ny = d->Ny; p.Nz = d->Nz;
    p.max_weight = d->max_weight; p.carve = d->carve != 0;
    p.gx = (float)d->origin[0]; p.gy = (float)d->origin[1]; p.gz = (float)d->origin[2];
    p.vs = (float)d->voxel_size; p.trunc = (float)d->trunc;

    // blocks of 64 x 4 voxels in (i, j); rows and slices beyond the grid limits, and slices beyond 2^22 blocks, are walked in grid strides
    const long long gx = (d->Nx + 63) / 64;
    long long gy = (d->Ny + kRasterWaves - 1) / kRasterWaves;
    if (gy > 65535) gy = 65535;
    long long gz = (1LL << 22) / (gx * gy);
    if (gz > d->Nz) gz = d->Nz;
    if (gz > 65535) gz = 65535;
    if (gz < 1) gz = 1;
    const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)gz), block(kRasterThreads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return by_image_dtype(d->cloud.image_dtype, "tsdf_integrate", [&](auto ti) {
        using IT = decltype(ti);
        return launch<tsdf_integrate_kernel<IT>>("tsdf_integrate", grid, block, 0, s, p);
    });
}

static int tsdf_extract_impl(const s2m2_tsdf_extract_desc* d, void* stream) {
    S2M2_REQUIRE(d != nullptr, "tsdf_extract: null descriptor");
    if (int rc = refuse_while_recording("tsdf_extract")) return rc;
    TsdfExtractParams p;
    if (int rc = tsdf_extract_params("tsdf_extract", d, true, p)) return rc;
    S2M2_REQUIRE(d->workspace != nullptr, "tsdf_extract: null workspace (s2m2_tsdf_workspace_bytes)");
    S2M2_REQUIRE(((uintptr_t)d->workspace & 3) == 0, "tsdf_extract: the workspace must be 4-byte aligned");
    p.tile_counts = static_cast<int*>(d->workspace);

    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(p.tiles), block(kRasterThreads);
    if (int rc = launch<tsdf_count_kernel>("tsdf_extract (count)", grid, block, 0, s, p)) return rc;
    return launch<tsdf_store_kernel>("tsdf_extract (store)", grid, block, 0, s, p);
}

}  // namespace s2m2

extern "C" int s2m2_tsdf_tile_voxels(int Nx, int Ny, int Nz) { return s2m2::tsdf_dims_ok(Nx, Ny, Nz) ? s2m2::kTsdfTileVoxels : 0; }

extern "C" size_t s2m2_tsdf_workspace_bytes(int Nx, int Ny, int Nz) {
    using namespace s2m2;
    if (!tsdf_dims_ok(Nx, Ny, Nz)) return 0;
    const long long n = (long long)Nx * Ny * Nz;
    return round256((size_t)((n + kTsdfTileVoxels - 1) / kTsdfTileVoxels) * sizeof(int));
}

extern "C" int s2m2_tsdf_integrate(const s2m2_tsdf_desc* desc, void* stream) { return s2m2::tsdf_integrate_impl(desc, stream); }

extern "C" int s2m2_tsdf_extract(const s2m2_tsdf_extract_desc* desc, void* stream) { return s2m2::tsdf_extract_impl(desc, stream); }
