// K20: the surface mesh behind the 3D stage (include/s2m2_hip.h: s2m2_mesh) -- K15's vertices plus the triangles that connect neighbouring kept
// pixels of similar disparity, both compacted in raster order.  Three launches without a host step, atomics or waiting between blocks:
//   mesh_count_kernel   a block owns a tile of whole image rows and reads one halo row below it: dense depth / mask, the number of kept pixels
//                       and the number of faces of the tile's quads into the workspace
//   (vertices)          K15's scatter kernel itself (cloud.hip: cloud_scatter_kernel with the rank-map option) on K20's tiles: the records, and
//                       the rank of every pixel (-1: not kept) into the dense rank map: `index`, or the workspace without it
//   mesh_face_kernel    prefix over the tile face counts, the face rule again from disp and the rank map (rank >= 0 <=> keep), ranks of the
//                       two candidate slots of every quad (raster_rank_step), 12-byte stores (ranks run by lane, then by quad and slot: a
//                       thread's up to eight faces lie back to back and the faces of a wave's step fill one contiguous range)
// A quad belongs to the thread that owns its top-left pixel (raster_tiles.h: four consecutive pixels per thread).  Its right-hand column is the
// first pixel of the next lane (a shuffle); the last lane of a wave reads that pixel itself.  The row below is read by the same thread with the
// same loads (it is the tile's own next row, or the halo row: served by the cache, not by HBM).
#include "cloud_device.h"
#include "launch.h"
#include "plan.h"

namespace s2m2 {

// A tile: as many whole rows as fit (at least one).  Half of K15's: the steps of a block run one after the other (every step waits for its
// loads, then for the barrier of the ranks), and at 1216x1024 the three launches take 51 us with one row per tile, 78 us with three, 122 us
// with six (profiles/mesh/tile_size.txt); below one row per tile nothing is left to gain, and 2432x2048 does not depend on it
constexpr int kMeshTilePixels = 2048;

// keep, disparity and (face kernel) rank of the 2 x 5 pixels behind a thread's four quads: [row][column], column 4 = the next lane's first pixel
struct Corners {
    bool k[2][5];
    float d[2][5];
};

__device__ __forceinline__ bool mesh_joined(const Corners& q, int r0, int c0, int r1, int c1, float max_jump) {
    return q.k[r0][c0] && q.k[r1][c1] && fabsf(q.d[r0][c0] - q.d[r1][c1]) <= max_jump;
}

// the face rule of the header for the quad whose top-left pixel is column j: which diagonal, and which of the two candidate slots are emitted.
// A candidate is emitted iff its three edges are joined, which needs its three corners kept: with three corners kept only the candidate that
// avoids the missing one can pass, and it is found in the diagonal's family that has it (e or a missing: b-c; b or c missing: a-e).
__device__ __forceinline__ void mesh_quad(const Corners& q, int j, float max_jump, bool& diag_ae, bool& f0, bool& f1) {
    const bool all = q.k[0][j] && q.k[0][j + 1] && q.k[1][j] && q.k[1][j + 1];
    diag_ae = all ? fabsf(q.d[0][j] - q.d[1][j + 1]) <= fabsf(q.d[0][j + 1] - q.d[1][j]) : !(q.k[0][j + 1] && q.k[1][j]);
    const bool ac = mesh_joined(q, 0, j, 1, j, max_jump), ab = mesh_joined(q, 0, j, 0, j + 1, max_jump);
    const bool ce = mesh_joined(q, 1, j, 1, j + 1, max_jump), be = mesh_joined(q, 0, j + 1, 1, j + 1, max_jump);
    const bool ae = mesh_joined(q, 0, j, 1, j + 1, max_jump), bc = mesh_joined(q, 0, j + 1, 1, j, max_jump);
    f0 = diag_ae ? (ac && ce && ae) : (ac && bc && ab);          // (a,c,e) : (a,c,b)
    f1 = diag_ae ? (ae && be && ab) : (bc && ce && be);          // (a,e,b) : (b,c,e)
}

// column 4 of both rows: lanes 0..62 take the next lane's first pixel, lane 63 its own copy `own` (valid in lane 63 only)
__device__ __forceinline__ float mesh_from_right(float first, float own) {
    const float s = __shfl_down(first, 1, 64);
    return (threadIdx.x & 63) == 63 ? own : s;
}

// count kernel: keep and disparity of rows v and v + 1 from the maps.  Block-uniform call (shuffles inside).
template <bool VEC>
__device__ __forceinline__ void mesh_corners_from_maps(const CloudParams& p, int b, int v, int u0, const float z0[4], const float d0[4], Corners& q) {
    float z[2][5], d[2][5];
#pragma unroll
    for (int j = 0; j < 4; ++j) { z[0][j] = z0[j]; d[0][j] = d0[j]; z[1][j] = 0.f; d[1][j] = 0.f; }
    const bool below = v + 1 < p.H;
    if (below && u0 < p.W) cloud_eval4d<VEC>(p, b, v + 1, u0, z[1], d[1]);
    // lane 63: the pixel right of its group, from the maps
    float zr[2] = {0.f, 0.f}, dr[2] = {0.f, 0.f};
    const int ur = u0 + 4;
    if ((threadIdx.x & 63) == 63 && ur < p.W) {          // ur >= 1: u0 >= -3
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 0 || below) {
                const size_t m = raster_map_index(p, b, v + r, ur);
                dr[r] = p.disp[m];
                zr[r] = cloud_z(p, dr[r], p.occ[m], p.conf[m]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        z[r][4] = mesh_from_right(z[r][0], zr[r]);
        d[r][4] = mesh_from_right(d[r][0], dr[r]);
#pragma unroll
        for (int j = 0; j < 5; ++j) { q.k[r][j] = z[r][j] > 0.f; q.d[r][j] = d[r][j]; }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kRasterThreads) void mesh_count_kernel(const MeshParams mp) {
    __shared__ int red_v[kRasterWaves], red_f[kRasterWaves];
    const CloudParams& p = mp.c;
    const int b = blockIdx.y, tile = blockIdx.x;
    int n = 0, nf = 0;
    for (RasterWalk w(p, tile, p.H); w.more(); w.next()) {                // (shuffles inside)
        const int v = w.v, u0 = w.u0();
        float z[4] = {0.f, 0.f, 0.f, 0.f}, d[4] = {0.f, 0.f, 0.f, 0.f};
        if (u0 < p.W) cloud_eval4d<VEC>(p, b, v, u0, z, d);
#pragma unroll
        for (int j = 0; j < 4; ++j) n += z[j] > 0.f;
        Corners q;
        mesh_corners_from_maps<VEC>(p, b, v, u0, z, d, q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bool diag_ae, f0, f1;
            mesh_quad(q, j, mp.max_jump, diag_ae, f0, f1);
            nf += (int)f0 + (int)f1;
        }
        if (u0 < p.W) cloud_store_dense<VEC>(p, b, v, u0, z);
    }
    n = block_sum_int(n, red_v);
    nf = block_sum_int(nf, red_f);
    if (threadIdx.x == 0) {
        p.tile_counts[(size_t)b * p.tiles + tile] = n;
        mp.tile_faces[(size_t)b * p.tiles + tile] = nf;
    }
}

// face kernel: disparity and rank of the thread's four pixels of image row v (pixels outside the row keep d = 0, rank -1)
template <bool VEC>
__device__ __forceinline__ void mesh_load4(const MeshParams& mp, int b, int v, int u0, float d[4], int rk[4]) {
    map_load4<VEC>(mp.c.disp, raster_map_index(mp.c, b, v, u0), u0, mp.c.W, d);
    dense_load4(mp.rank, raster_dense_row(mp.c, b, v), u0, mp.c.W, mp.rank_vec != 0, rk);
}

struct __attribute__((packed, aligned(4))) MeshFace { int a, b, c; };

template <bool VEC>
__global__ __launch_bounds__(kRasterThreads) void mesh_face_kernel(const MeshParams mp) {
    __shared__ int red[kRasterWaves];
    __shared__ int wave_n[2][kRasterWaves];
    const CloudParams& p = mp.c;
    const int b = blockIdx.y, tile = blockIdx.x;
    const int lane = threadIdx.x & 63;
    long long base = tile_prefix(mp.tile_faces + (size_t)b * p.tiles, tile, red);
    MeshFace* faces = reinterpret_cast<MeshFace*>(mp.faces) + (size_t)b * (size_t)mp.face_capacity;
    int step = 0;
    for (RasterWalk w(p, tile, p.H - 1); w.more(); w.next()) {            // the last image row has no quads; (shuffles inside)
        const int v = w.v, u0 = w.u0();
        float d[2][5];
        int rk[2][5];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { d[r][j] = 0.f; rk[r][j] = -1; }
            if (u0 < p.W) mesh_load4<VEC>(mp, b, v + r, u0, d[r], rk[r]);
            float dr = 0.f;
            int rr = -1;
            const int ur = u0 + 4;
            if (lane == 63 && ur < p.W) {
                dr = p.disp[raster_map_index(p, b, v + r, ur)];
                rr = mp.rank[raster_dense_row(p, b, v + r) + ur];
            }
            d[r][4] = mesh_from_right(d[r][0], dr);
            rk[r][4] = __builtin_bit_cast(int, mesh_from_right(__builtin_bit_cast(float, rk[r][0]), __builtin_bit_cast(float, rr)));
        }
        Corners q;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 5; ++j) { q.k[r][j] = rk[r][j] >= 0; q.d[r][j] = d[r][j]; }
        bool diag[4], f[8];                                                // f: by quad, then by slot
#pragma unroll
        for (int j = 0; j < 4; ++j) mesh_quad(q, j, mp.max_jump, diag[j], f[2 * j], f[2 * j + 1]);
        long long r = raster_rank_step(f, wave_n, step++, base);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ra = rk[0][j], rb = rk[0][j + 1], rc = rk[1][j], re = rk[1][j + 1];
            if (f[2 * j]) {
                if (r < mp.face_capacity) { MeshFace t = {ra, rc, diag[j] ? re : rb}; faces[r] = t; }
                ++r;
            }
            if (f[2 * j + 1]) {
                if (r < mp.face_capacity) { MeshFace t = {diag[j] ? ra : rb, diag[j] ? re : rc, diag[j] ? rb : re}; faces[r] = t; }
                ++r;
            }
        }
    }
    if (tile == p.tiles - 1 && threadIdx.x == 0) mp.face_count[b] = (int)base;
}

// faces of a pair fit an int32 count: 2 (H-1) (W-1) < 2^31
static bool mesh_extents_ok(int B, int H, int W) { return raster_extents_ok(B, H, W, 1LL << 30); }

static int mesh_tile_rows(int W) { return tile_rows(W, kMeshTilePixels); }

static size_t mesh_counts_bytes(int B, int H, int W) { return round256(2 * (size_t)B * tiles(H, mesh_tile_rows(W)) * sizeof(int)); }

static int mesh_impl(const s2m2_mesh_desc* d, void* stream) {
    S2M2_REQUIRE(d != nullptr, "mesh: null descriptor");
    if (int rc = refuse_while_recording("mesh")) return rc;
    const s2m2_cloud_desc* cd = &d->cloud;
    if (d->face_count == nullptr) return s2m2_cloud(cd, stream);           // no mesh requested: K15 on the same fields
    S2M2_REQUIRE(cd->count != nullptr, "mesh: face_count comes with count (the faces index the vertex records)");
    MeshParams mp;
    bool vec = false;
    if (int rc = cloud_validate(cd, "mesh", kMeshTilePixels, mp.c, vec)) return rc;       // K20's own tile geometry
    S2M2_REQUIRE(mesh_extents_ok(cd->B, cd->H, cd->W), "mesh: extents too large (H*W < 2^30)");
    S2M2_REQUIRE(d->face_capacity >= 0, "mesh: negative face_capacity %lld", d->face_capacity);
    S2M2_REQUIRE(d->faces != nullptr || d->face_capacity == 0, "mesh: null pointer (faces) with face_capacity %lld", d->face_capacity);
    S2M2_REQUIRE(((uintptr_t)d->faces & 3) == 0 && ((uintptr_t)d->index & 3) == 0 && ((uintptr_t)d->face_count & 3) == 0,
                 "mesh: faces, face_count and index must be 4-byte aligned");
    S2M2_REQUIRE(d->max_jump >= 0.0, "mesh: max_jump must be >= 0 (+inf is allowed), got %g", d->max_jump);       // false for NaN

    const size_t counts_bytes = mesh_counts_bytes(cd->B, cd->H, cd->W);
    mp.tile_faces = mp.c.tile_counts + (size_t)cd->B * mp.c.tiles;
    mp.rank = d->index ? d->index : reinterpret_cast<int*>(static_cast<char*>(cd->workspace) + counts_bytes);
    mp.rank_vec = ((uintptr_t)mp.rank & 15) == 0;
    mp.faces = static_cast<int*>(d->faces);
    mp.face_count = d->face_count;
    mp.face_capacity = d->face_capacity;
    mp.max_jump = (float)d->max_jump;

    const dim3 grid(mp.c.tiles, cd->B), block(kRasterThreads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = vec ? launch<mesh_count_kernel<true>>("mesh (count)", grid, block, 0, s, mp) : launch<mesh_count_kernel<false>>("mesh (count)", grid, block, 0, s, mp))
        return rc;
    if (int rc = mesh_vertices(mp, vec, cd->image_dtype, grid, s)) return rc;
    return vec ? launch<mesh_face_kernel<true>>("mesh (faces)", grid, block, 0, s, mp) : launch<mesh_face_kernel<false>>("mesh (faces)", grid, block, 0, s, mp);
}

}  // namespace s2m2

extern "C" size_t s2m2_mesh_workspace_bytes(int B, int H, int W) {
    if (!s2m2::mesh_extents_ok(B, H, W)) return 0;
    return s2m2::mesh_counts_bytes(B, H, W) + s2m2::round256((size_t)B * H * W * sizeof(int));
}

extern "C" int s2m2_mesh_tile_rows(int H, int W) { return s2m2::mesh_extents_ok(1, H, W) ? s2m2::mesh_tile_rows(W) : 0; }

extern "C" int s2m2_mesh(const s2m2_mesh_desc* desc, void* stream) { return s2m2::mesh_impl(desc, stream); }
