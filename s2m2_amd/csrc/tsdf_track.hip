// K27: the camera tracked against K24's volume -- frame-to-model point-to-plane ICP with projective data association (include/s2m2_hip.h:
// s2m2_tsdf_track).  The live frame is K15's maps, the model K26's depth and gradient maps; the refined pose goes into the DEVICE pose buffer
// that K24 and K26 read next.  Two launches per iteration, no host step, no floating-point atomics:
//   tsdf_track_sums_kernel    a block owns a tile of K15's raster walk (raster_tiles.h: four pixels per thread, 4096 per tile).  Per
//                             pixel: K15's keep and z (cloud_device.h), the point moved to the world with the pose of the pair (uniform loads), projected into the model
//                             camera, four gathered reads (depth and the three gradient planes; the sixteen of a thread's four pixels are
//                             issued together), the gate, and the row (J, r) in fp32 with one rounding per operation.  The 28 products and
//                             the count are summed in double: a thread over its pixels, then the block through LDS (eight groups of 32
//                             threads in ascending order, then the groups in order), one 32-double partial per tile into the workspace.
//                             The last iteration also writes the residual map.
//   tsdf_track_solve_kernel   one block per pair: the partials are summed in a fixed order (eight strided groups, then the groups in order),
//                             one thread runs the 6 x 6 Cholesky, Rodrigues' formula and the update in double, and writes the pose (status 0
//                             alone) and the row of `systems`.
// The order of every addition depends on the shapes alone: bit-reproducible.
#include "cloud_device.h"
#include "launch.h"
#include "plan.h"
#include "tsdf_device.h"

namespace s2m2 {

constexpr int kTrackRow = 32;                            // doubles of a partial and of a row of `systems`
constexpr int kTrackSums = 28;                           // 21 + 6 + 1
constexpr int kTrackGroups = kRasterThreads / kTrackRow; // strided groups of the solve launch's pass over the partials
constexpr int kTrackMaxIters = 64;
constexpr int kTrackTilePixels = kCloudTilePixels;       // K15's tile.  Measured: with tiles of 1024 pixels 640 x 480 gains 4 us per iteration and
                                                         // 1216 x 1024 loses 13 (a row is then a tile of two steps, and every block pays the epilogue)
constexpr unsigned kTrackHole = 0x7fc00000u;             // residual of a pixel without a correspondence

struct TsdfTrackParams {
    CloudParams c;              // the inputs of K15 (its outputs are null)
    float* poses;               // (B, 12) on the device: read by both launches, written by the solve launch
    const float* model_poses;
    const float* model_depth;
    const float* model_gradients;
    double* partials;           // (B, tiles, 32): the workspace
    double* systems;            // this iteration's row of pair 0, or null
    float* residual;            // null but in the last iteration
    long long systems_stride;   // doubles from a pair's row to the next pair's: n_iters * 32
    int Ht, Wt;
    int residual_vec;
    int min_count;
    float mfx, mfy, mcx, mcy, max_dist2;
    double max_rot, max_trans;
};

// The rule of one kept live pixel (v, u) at depth z in two halves, so that a thread issues the gathers of its four pixels together instead of
// one dependent round trip after the other.  q = the pair's pose, m = its model pose.  One IEEE rounding per operation.
struct TrackPoint {
    float px, py, pz;           // the live point in the world
    float fu, fv;               // its pixel in the model image
};

// the point moved to the world and projected into the model camera: false where the rule skips it before the model maps are read
__device__ __forceinline__ bool track_project(const TsdfTrackParams& p, const float (&q)[12], const float (&m)[12], int v, int u, float z, TrackPoint& t) {
#pragma clang fp contract(off)
    float x, y;
    cloud_xy(p.c, v, u, z, x, y);
    const float c0 = x - q[3], c1 = y - q[7], c2 = z - q[11];
    t.px = (q[0] * c0 + q[4] * c1) + q[8] * c2;
    t.py = (q[1] * c0 + q[5] * c1) + q[9] * c2;
    t.pz = (q[2] * c0 + q[6] * c1) + q[10] * c2;
    const float X = ((m[0] * t.px + m[1] * t.py) + m[2] * t.pz) + m[3];
    const float Y = ((m[4] * t.px + m[5] * t.py) + m[6] * t.pz) + m[7];
    const float Z = ((m[8] * t.px + m[9] * t.py) + m[10] * t.pz) + m[11];
    t.fu = 0.f; t.fv = 0.f;
    if (!(Z > 0.f && Z < INFINITY)) return false;
    const float up = (p.mfx * X) / Z + p.mcx;
    const float vp = (p.mfy * Y) / Z + p.mcy;
    t.fu = rintf(up); t.fv = rintf(vp);
    return t.fu >= 0.f && t.fu < (float)p.Wt && t.fv >= 0.f && t.fv < (float)p.Ht;                // a NaN fails; both now fit an int
}

// the row (J, r) from the model's depth dm and gradient g at the point's pixel: false where the rule skips it
__device__ __forceinline__ bool track_finish(const TsdfTrackParams& p, const float (&m)[12], const TrackPoint& t, float dm, float gx, float gy, float gz,
                                             float (&J)[6], float& r) {
#pragma clang fp contract(off)
    if (!(dm > 0.f)) return false;
    const float s = (gx * gx + gy * gy) + gz * gz;
    if (!(s > 0.f && s < INFINITY)) return false;
    const float len = sqrtf(s);
    const float nx = gx / len, ny = gy / len, nz = gz / len;
    const float mx = (t.fu - p.mcx) * dm / p.mfx;
    const float my = (t.fv - p.mcy) * dm / p.mfy;
    const float e0 = mx - m[3], e1 = my - m[7], e2 = dm - m[11];
    const float wx = (m[0] * e0 + m[4] * e1) + m[8] * e2;
    const float wy = (m[1] * e0 + m[5] * e1) + m[9] * e2;
    const float wz = (m[2] * e0 + m[6] * e1) + m[10] * e2;
    const float dx = wx - t.px, dy = wy - t.py, dz = wz - t.pz;
    if (!((dx * dx + dy * dy) + dz * dz <= p.max_dist2)) return false;
    r = (nx * dx + ny * dy) + nz * dz;
    J[0] = t.py * nz - t.pz * ny;
    J[1] = t.pz * nx - t.px * nz;
    J[2] = t.px * ny - t.py * nx;
    J[3] = nx; J[4] = ny; J[5] = nz;
    return true;
}

template <bool VEC>
__global__ __launch_bounds__(kRasterThreads) void tsdf_track_sums_kernel(const TsdfTrackParams p) {
    __shared__ double all[kTrackSums + 1][kRasterThreads + 1];
    __shared__ double grp[kTrackGroups][kTrackRow];
    const CloudParams& c = p.c;
    const int b = blockIdx.y, tile = blockIdx.x;
    float q[12], m[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        q[i] = p.poses[(size_t)b * 12 + i];
        m[i] = p.model_poses[(size_t)b * 12 + i];
    }
    const size_t mplane = (size_t)p.Ht * p.Wt;
    const float* md = p.model_depth + (size_t)b * mplane;
    const float* mg = p.model_gradients + (size_t)b * 3 * mplane;
    double acc[kTrackSums];
#pragma unroll
    for (int i = 0; i < kTrackSums; ++i) acc[i] = 0.0;
    int n = 0;
    for (RasterWalk w(c, tile, c.H); w.more(); w.next()) {
        const int v = w.v, u0 = w.u0();
        if (u0 >= c.W) continue;
        float z[4], res[4];
        cloud_eval4<VEC>(c, b, v, u0, z);
        // the four gathers of each of the four pixels, issued together: a pixel without a model pixel reads element 0 and drops it
        TrackPoint t[4];
        bool in[4];
        float dm[4], gx[4], gy[4], gz[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) in[j] = z[j] > 0.f && track_project(p, q, m, v, u0 + j, z[j], t[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t pix = in[j] ? (size_t)(int)t[j].fv * p.Wt + (int)t[j].fu : 0;
            dm[j] = md[pix];
            gx[j] = mg[pix]; gy[j] = mg[mplane + pix]; gz[j] = mg[2 * mplane + pix];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float J[6], r = 0.f;
            const bool ok = in[j] && track_finish(p, m, t[j], dm[j], gx[j], gy[j], gz[j], J, r);
            res[j] = ok ? r : __builtin_bit_cast(float, kTrackHole);
            if (ok) {
                const double Jd[7] = {(double)J[0], (double)J[1], (double)J[2], (double)J[3], (double)J[4], (double)J[5], (double)r};
                int k = 0;
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int jj = i; jj < 6; ++jj) acc[k++] += Jd[i] * Jd[jj];       // exact products: one rounding per addition, fused or not
#pragma unroll
                for (int i = 0; i < 7; ++i) acc[21 + i] += Jd[i] * Jd[6];
                ++n;
            }
        }
        if (p.residual) dense_store4(p.residual, raster_dense_row(c, b, v), u0, c.W, p.residual_vec != 0, res);
    }
    // the block's sums: every thread's 29 values through LDS (a row per sum, padded so that the 32 sums a half-wave reads lie in 32 banks);
    // thread (g, e) adds the 32 threads 32 g .. 32 g + 31 of sum e in ascending order, then the eight groups are added in order
#pragma unroll
    for (int i = 0; i < kTrackSums; ++i) all[i][threadIdx.x] = acc[i];
    all[kTrackSums][threadIdx.x] = (double)n;
    __syncthreads();
    const int e = threadIdx.x & (kTrackRow - 1), g = threadIdx.x / kTrackRow;
    double s = 0.0;
    if (e <= kTrackSums) {
#pragma unroll 8
        for (int k = 0; k < kTrackRow; ++k) s += all[e][g * kTrackRow + k];
    }
    grp[g][e] = s;
    __syncthreads();
    if (threadIdx.x < kTrackRow) {
        double t = grp[0][e];
#pragma unroll
        for (int k = 1; k < kTrackGroups; ++k) t += grp[k][e];
        p.partials[((size_t)b * c.tiles + tile) * kTrackRow + e] = t;           // [29 .. 31] = 0
    }
}

__device__ __forceinline__ bool track_finite(double x) { return fabs(x) < (double)INFINITY; }

__global__ __launch_bounds__(kRasterThreads) void tsdf_track_solve_kernel(const TsdfTrackParams p) {
    __shared__ double grp[kTrackGroups][kTrackRow];
    __shared__ double sys[kTrackRow];
    const int b = blockIdx.x;
    const int e = threadIdx.x & (kTrackRow - 1), g = threadIdx.x / kTrackRow;
    const double* part = p.partials + (size_t)b * p.c.tiles * kTrackRow;
    double s = 0.0;
    for (int t = g; t < p.c.tiles; t += kTrackGroups) s += part[(size_t)t * kTrackRow + e];
    grp[g][e] = s;
    __syncthreads();
    if (threadIdx.x < kTrackRow) {
        double a = grp[0][e];
#pragma unroll
        for (int k = 1; k < kTrackGroups; ++k) a += grp[k][e];
        sys[e] = a;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;

    double A[6][6], rhs[6], xi[6] = {0, 0, 0, 0, 0, 0};
    {
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) { A[i][j] = sys[k]; A[j][i] = sys[k]; ++k; }
#pragma unroll
        for (int i = 0; i < 6; ++i) rhs[i] = sys[21 + i];
    }
    const double count = sys[28];
    int status = 0;
    double wn = 0.0, vn = 0.0;
    float out[12];
    float* pose = p.poses + (size_t)b * 12;
    if (count < (double)p.min_count) {
        status = 1;
    } else {
        bool fin = true;
#pragma unroll
        for (int i = 0; i < kTrackSums; ++i) fin = fin && track_finite(sys[i]);
        if (!fin) status = 2;
    }
    if (status == 0) {
        // Cholesky A = L L^T, L in the lower triangle of A
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double d = A[j][j];
#pragma unroll
            for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
            if (!(d > 0.0 && track_finite(d))) { ok = false; d = 1.0; }
            const double l = 1.0 / sqrt(d);                                  // the diagonal holds 1 / L[j][j]: one division per column
            A[j][j] = l;
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double x = A[i][j];
#pragma unroll
                for (int k = 0; k < j; ++k) x -= A[i][k] * A[j][k];
                A[i][j] = x * l;
            }
        }
        double yv[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double x = rhs[i];
#pragma unroll
            for (int k = 0; k < i; ++k) x -= A[i][k] * yv[k];
            yv[i] = x * A[i][i];
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {
            double x = yv[i];
#pragma unroll
            for (int k = i + 1; k < 6; ++k) x -= A[k][i] * xi[k];
            xi[i] = x * A[i][i];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) ok = ok && track_finite(xi[i]);
        if (!ok) status = 2;
    }
    if (status == 0) {
        wn = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]);
        vn = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
        if (wn > p.max_rot || vn > p.max_trans) status = 3;
    }
    if (status == 0) {
        const double th2 = wn * wn;
        double ca, cb;
        if (wn < 1e-4) { ca = 1.0 - th2 / 6.0; cb = 0.5 - th2 / 24.0; }
        else { ca = sin(wn) / wn; cb = (1.0 - cos(wn)) / th2; }
        const double K[3][3] = {{0.0, -xi[2], xi[1]}, {xi[2], 0.0, -xi[0]}, {-xi[1], xi[0], 0.0}};
        double E[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double k2 = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
                E[i][j] = ((i == j ? 1.0 : 0.0) + ca * K[i][j]) + cb * k2;
            }
        double R[3][3], t[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            t[i] = (double)pose[4 * i + 3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                // (R E^T)[i][j] = sum_k R[i][k] E[j][k]
                R[i][j] = ((double)pose[4 * i] * E[j][0] + (double)pose[4 * i + 1] * E[j][1]) + (double)pose[4 * i + 2] * E[j][2];
            }
        }
        const double n0 = sqrt((R[0][0] * R[0][0] + R[0][1] * R[0][1]) + R[0][2] * R[0][2]);
#pragma unroll
        for (int j = 0; j < 3; ++j) R[0][j] = R[0][j] / n0;
        const double dot = (R[0][0] * R[1][0] + R[0][1] * R[1][1]) + R[0][2] * R[1][2];
#pragma unroll
        for (int j = 0; j < 3; ++j) R[1][j] = R[1][j] - dot * R[0][j];
        const double n1 = sqrt((R[1][0] * R[1][0] + R[1][1] * R[1][1]) + R[1][2] * R[1][2]);
#pragma unroll
        for (int j = 0; j < 3; ++j) R[1][j] = R[1][j] / n1;
        R[2][0] = R[0][1] * R[1][2] - R[0][2] * R[1][1];
        R[2][1] = R[0][2] * R[1][0] - R[0][0] * R[1][2];
        R[2][2] = R[0][0] * R[1][1] - R[0][1] * R[1][0];
        bool fin = true;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double ti = t[i] - ((R[i][0] * xi[3] + R[i][1] * xi[4]) + R[i][2] * xi[5]);
#pragma unroll
            for (int j = 0; j < 3; ++j) out[4 * i + j] = (float)R[i][j];
            out[4 * i + 3] = (float)ti;
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) fin = fin && fabsf(out[i]) < INFINITY;
        if (!fin) status = 2;
    }
    if (status == 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) pose[i] = out[i];
    }
    if (p.systems) {
        double* row = p.systems + (size_t)b * p.systems_stride;
#pragma unroll
        for (int i = 0; i < 29; ++i) row[i] = sys[i];
        row[29] = (double)status;
        row[30] = (status == 0 || status == 3) ? wn : 0.0;
        row[31] = (status == 0 || status == 3) ? vn : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host

static int tsdf_track_impl(const s2m2_tsdf_track_desc* d, void* stream) {
    S2M2_REQUIRE(d != nullptr, "tsdf_track: null descriptor");
    if (int rc = refuse_while_recording("tsdf_track")) return rc;
    TsdfTrackParams p;
    bool vec = false;
    s2m2_cloud_desc in = d->cloud;                  // the inputs alone: the output fields of the embedded descriptor are ignored
    in.depth = nullptr; in.mask = nullptr; in.records = nullptr; in.count = nullptr; in.workspace = nullptr; in.capacity = 0;
    if (int rc = cloud_validate(&in, "tsdf_track", kTrackTilePixels, p.c, vec, false)) return rc;
    S2M2_REQUIRE(d->poses && d->model_poses, "tsdf_track: null pointer (poses / model_poses)");
    S2M2_REQUIRE(d->model_depth && d->model_gradients, "tsdf_track: null pointer (model_depth / model_gradients)");
    S2M2_REQUIRE((((uintptr_t)d->poses | (uintptr_t)d->model_poses | (uintptr_t)d->model_depth | (uintptr_t)d->model_gradients) & 3) == 0,
                 "tsdf_track: poses, model_poses, model_depth and model_gradients must be 4-byte aligned");
    S2M2_REQUIRE(d->workspace != nullptr, "tsdf_track: null workspace (s2m2_tsdf_track_workspace_bytes)");
    S2M2_REQUIRE(((uintptr_t)d->workspace & 7) == 0, "tsdf_track: the workspace must be 8-byte aligned");
    S2M2_REQUIRE(d->Ht > 0 && d->Wt > 0, "tsdf_track: non-positive model extents Ht=%d Wt=%d", d->Ht, d->Wt);
    S2M2_REQUIRE((long long)d->Ht * d->Wt < (1LL << 31) && (long long)d->cloud.B * ((long long)d->Ht * d->Wt) < (1LL << 31),
                 "tsdf_track: model extents too large (B*Ht*Wt < 2^31)");
    S2M2_REQUIRE(tsdf_finite_f32(d->mfx) && tsdf_finite_f32(d->mfy) && (float)d->mfx != 0.f && (float)d->mfy != 0.f,
                 "tsdf_track: mfx and mfy must be finite and non-zero in fp32 (mfx=%g mfy=%g)", d->mfx, d->mfy);
    S2M2_REQUIRE(tsdf_finite_f32(d->mcx) && tsdf_finite_f32(d->mcy), "tsdf_track: mcx and mcy must be finite (also in fp32)");
    S2M2_REQUIRE(tsdf_positive_f32(d->max_dist) && tsdf_positive_f32(d->max_rot) && tsdf_positive_f32(d->max_trans),
                 "tsdf_track: max_dist, max_rot and max_trans must be finite and > 0 in fp32 (%g, %g, %g)", d->max_dist, d->max_rot, d->max_trans);
    S2M2_REQUIRE(d->min_count >= 6, "tsdf_track: min_count must be >= 6 (%d)", d->min_count);
    S2M2_REQUIRE(d->n_iters >= 1 && d->n_iters <= kTrackMaxIters, "tsdf_track: n_iters must be 1..%d (%d)", kTrackMaxIters, d->n_iters);
    S2M2_REQUIRE(((uintptr_t)d->systems & 7) == 0, "tsdf_track: systems must be 8-byte aligned");
    S2M2_REQUIRE(((uintptr_t)d->residual & 3) == 0, "tsdf_track: residual must be 4-byte aligned");

    p.poses = d->poses; p.model_poses = d->model_poses;
    p.model_depth = d->model_depth; p.model_gradients = d->model_gradients;
    p.partials = static_cast<double*>(d->workspace);
    p.systems_stride = (long long)d->n_iters * kTrackRow;
    p.Ht = d->Ht; p.Wt = d->Wt;
    p.residual_vec = ((uintptr_t)d->residual & 15) == 0;
    p.min_count = d->min_count;
    p.mfx = (float)d->mfx; p.mfy = (float)d->mfy; p.mcx = (float)d->mcx; p.mcy = (float)d->mcy;
    const float max_dist = (float)d->max_dist;
    p.max_dist2 = max_dist * max_dist;
    p.max_rot = d->max_rot; p.max_trans = d->max_trans;

    const dim3 grid(p.c.tiles, d->cloud.B), block(kRasterThreads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int it = 0; it < d->n_iters; ++it) {
        p.systems = d->systems ? d->systems + (size_t)it * kTrackRow : nullptr;
        p.residual = it == d->n_iters - 1 ? d->residual : nullptr;
        if (int rc = vec ? launch<tsdf_track_sums_kernel<true>>("tsdf_track (sums)", grid, block, 0, s, p)
                         : launch<tsdf_track_sums_kernel<false>>("tsdf_track (sums)", grid, block, 0, s, p))
            return rc;
        if (int rc = launch<tsdf_track_solve_kernel>("tsdf_track (solve)", dim3(d->cloud.B), block, 0, s, p)) return rc;
    }
    return 0;
}

}  // namespace s2m2

extern "C" size_t s2m2_tsdf_track_workspace_bytes(int B, int H, int W) {
    using namespace s2m2;
    if (!raster_extents_ok(B, H, W)) return 0;
    return round256((size_t)B * tiles(H, tile_rows(W, kTrackTilePixels)) * kTrackRow * sizeof(double));
}

extern "C" int s2m2_tsdf_track(const s2m2_tsdf_track_desc* desc, void* stream) { return s2m2::tsdf_track_impl(desc, stream); }
