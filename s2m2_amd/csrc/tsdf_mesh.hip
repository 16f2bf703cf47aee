// K25: the surface of a TSDF volume as a triangle mesh (include/s2m2_hip.h: s2m2_tsdf_mesh) -- marching cubes over the cells of K24's volume.
// The vertices are K24's surface points (tsdf_device.h: the same device functions as s2m2_tsdf_extract, so the same bytes); the faces join them
// by the generated case table of mc_table.h.  Three launches over K24's tiles of kTsdfTileVoxels consecutive voxels, a cell owned by the thread
// of its base voxel (i, j, k), so the lanes of a wave are 64 neighbours in i:
//   tsdf_mesh_count_kernel     per tile: its surface points (K24's count) and its faces (cell case -> the table's count)
//   tsdf_mesh_points_kernel    K24's store launch, which also writes the rank map: per voxel the rank of its first point
//   tsdf_mesh_faces_kernel     tile_prefix over the face counts, the cells evaluated again, a rank step over the per-thread face counts, and a
//                              face stored as three int32: the rank map of the edge's base voxel plus the emit flags of that voxel on the axes
//                              before the edge's (tsdf_crossings again: the voxel may lie outside the cell)
// Almost every cell has its eight signs alike or an unobserved corner and leaves before the table is touched.  The table (4 KB) is copied to LDS
// by every block: reading it from constant memory instead measured 1 - 5 % slower per call (profiles/tsdf/tsdfmesh.txt).  No atomics, no waiting between blocks: bit-reproducible.
#include "mc_table.h"
#include "tsdf_device.h"

namespace s2m2 {

static_assert(kRasterThreads == 256, "a thread copies one row of the case table");

struct TsdfMeshParams {
    TsdfExtractParams x;        // tile_counts: the points per tile
    int* face_tile_counts;      // the faces per tile
    int* rank_map;              // n ints
    int* faces;                 // (face_capacity, 3)
    int* face_count;
    long long face_capacity;
};

// the largest volume whose face count fits an int32 whatever its content
constexpr long long kTsdfMeshMaxVoxels = 2147483647LL / kMcMaxTriangles;

// the case of the cell whose corner 0 is voxel lin = (i, j, k): bit c set iff the tsdf at corner c = dx + 2 dy + 4 dz is negative; -1 where
// there is no such cell (a voxel of the grid's last layer along an axis) or it is not VALID (a corner is unobserved)
__device__ __forceinline__ int tsdf_cell_case(const TsdfExtractParams& p, int lin, int i, int j, int k) {
    if (i + 1 >= p.Nx || j + 1 >= p.Ny || k + 1 >= p.Nz) return -1;
    const int sy = p.Nx, sz = p.Nx * p.Ny;
    int cs = 0;
    bool valid = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float t;
        int w;
        tsdf_tw(p, lin + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz, t, w);
        valid = valid && w >= p.min_weight;
        cs |= (int)(t < 0.f) << c;
    }
    return valid ? cs : -1;
}

__device__ __forceinline__ bool tsdf_case_has_faces(int cs) { return cs > 0 && cs < 255; }

__global__ __launch_bounds__(kRasterThreads) void tsdf_mesh_count_kernel(const TsdfMeshParams m) {
    const TsdfExtractParams& p = m.x;
    __shared__ int red[2][kRasterWaves];
    __shared__ unsigned char triangles[256];
    triangles[threadIdx.x] = kMcTable[threadIdx.x][0];
    __syncthreads();
    const int tile = blockIdx.x;
    const int end = min(p.n, (tile + 1) * kTsdfTileVoxels);
    int nv = 0, nf = 0;
    for (int lin = tile * kTsdfTileVoxels + threadIdx.x; lin < end; lin += kRasterThreads) {
        int i, j, k;
        tsdf_coords(p, lin, i, j, k);
        float t0, t1[3];
        bool emit[3];
        tsdf_crossings(p, lin, i, j, k, t0, t1, emit);
        nv += (int)emit[0] + (int)emit[1] + (int)emit[2];
        const int cs = tsdf_cell_case(p, lin, i, j, k);
        if (tsdf_case_has_faces(cs)) nf += triangles[cs];
    }
    nv = block_sum_int(nv, red[0]);
    nf = block_sum_int(nf, red[1]);
    if (threadIdx.x == 0) {
        p.tile_counts[tile] = nv;
        m.face_tile_counts[tile] = nf;
    }
}

__global__ __launch_bounds__(kRasterThreads) void tsdf_mesh_points_kernel(const TsdfMeshParams m) {
    __shared__ int red[kRasterWaves];
    __shared__ int wave_n[2][kRasterWaves];
    tsdf_store_tile<true>(m.x, m.rank_map, red, wave_n);
}

// raster_rank_step (raster_tiles.h) for a COUNT per thread instead of flags: the rank of this thread's first item, `base` advanced by the
// block's total.  The same two-buffer hand-off of the wave totals behind one barrier; block-uniform call.
__device__ __forceinline__ long long tsdf_rank_counts(int cnt, int (*wave_n)[kRasterWaves], int step, long long& base) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = cnt;
    if (__ballot(cnt != 0) != 0ull) {                                   // wave-uniform; most waves hold no face at all
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
    }
    const int wave_total = __shfl(incl, 63, 64);
    if (lane == 0) wave_n[step & 1][wave] = wave_total;
    __syncthreads();
    long long r = base;
    int block_total = 0;
#pragma unroll
    for (int w = 0; w < kRasterWaves; ++w) {
        const int nw = wave_n[step & 1][w];
        if (w < wave) r += nw;
        block_total += nw;
    }
    base += block_total;
    return r + (incl - cnt);
}

__global__ __launch_bounds__(kRasterThreads) void tsdf_mesh_faces_kernel(const TsdfMeshParams m) {
    const TsdfExtractParams& p = m.x;
    __shared__ int red[kRasterWaves];
    __shared__ int wave_n[2][kRasterWaves];
    __shared__ unsigned char table[256][kMcRowBytes];
#pragma unroll
    for (int q = 0; q < kMcRowBytes; ++q) table[threadIdx.x][q] = kMcTable[threadIdx.x][q];
    const int tile = blockIdx.x;
    long long base = tile_prefix(m.face_tile_counts, tile, red);        // its barrier also publishes the table
    const int first = tile * kTsdfTileVoxels, end = min(p.n, first + kTsdfTileVoxels);
    const int sy = p.Nx, sz = p.Nx * p.Ny;
    int step = 0;
    for (int lin0 = first; lin0 < end; lin0 += kRasterThreads) {        // block-uniform: every thread takes every step
        const int lin = lin0 + threadIdx.x;
        int i = 0, j = 0, k = 0, cs = -1;
        if (lin < end) {
            tsdf_coords(p, lin, i, j, k);
            cs = tsdf_cell_case(p, lin, i, j, k);
        }
        const int nf = tsdf_case_has_faces(cs) ? table[cs][0] : 0;
        const long long r = tsdf_rank_counts(nf, wave_n, step++, base);
        for (int t = 0; t < nf && r + t < m.face_capacity; ++t) {
            int v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int e = table[cs][1 + 3 * t + c];                 // edge = (axis a, base corner b: the edge's number within a with a zero at bit a)
                const int a = e >> 2, q = e & 3;
                const int b = ((q >> a) << (a + 1)) | (q & ((1 << a) - 1));
                const int dx = b & 1, dy = (b >> 1) & 1, dz = b >> 2;
                const int vl = lin + dx + dy * sy + dz * sz;             // a corner of a cell: inside the grid
                int rank = m.rank_map[vl];
                if (a > 0) {                                            // the voxel's points on the axes before a come first
                    float t0, t1[3];
                    bool emit[3];
                    tsdf_crossings(p, vl, i + dx, j + dy, k + dz, t0, t1, emit);
                    rank += (int)emit[0] + (a > 1 ? (int)emit[1] : 0);
                }
                v[c] = rank;
            }
            int* f = m.faces + (size_t)(r + t) * 3;
            f[0] = v[0]; f[1] = v[1]; f[2] = v[2];
        }
    }
    if (tile == p.tiles - 1 && threadIdx.x == 0) *m.face_count = (int)base;
}

// ---------------------------------------------------------------------------------------------------------------- host

static bool tsdf_mesh_dims_ok(int Nx, int Ny, int Nz) { return tsdf_dims_ok(Nx, Ny, Nz) && (long long)Nx * Ny * Nz <= kTsdfMeshMaxVoxels; }

// the workspace: the points per tile and the faces per tile (one int each), then the rank map (one int per voxel)
static size_t tsdf_mesh_counts_bytes(long long n) { return round256((size_t)((n + kTsdfTileVoxels - 1) / kTsdfTileVoxels) * 2 * sizeof(int)); }

static int tsdf_mesh_impl(const s2m2_tsdf_mesh_desc* d, void* stream) {
    S2M2_REQUIRE(d != nullptr, "tsdf_mesh: null descriptor");
    if (int rc = refuse_while_recording("tsdf_mesh")) return rc;
    TsdfMeshParams m;
    if (int rc = tsdf_extract_params("tsdf_mesh", &d->extract, false, m.x)) return rc;
    S2M2_REQUIRE(d->face_count != nullptr, "tsdf_mesh: null pointer (face_count)");
    S2M2_REQUIRE((((uintptr_t)d->face_count | (uintptr_t)d->faces) & 3) == 0, "tsdf_mesh: faces and face_count must be 4-byte aligned");
    S2M2_REQUIRE(d->face_capacity >= 0, "tsdf_mesh: negative face_capacity %lld", d->face_capacity);
    S2M2_REQUIRE(d->faces || d->face_capacity == 0, "tsdf_mesh: null pointer (faces) with face_capacity %lld", d->face_capacity);
    S2M2_REQUIRE(tsdf_mesh_dims_ok(d->extract.Nx, d->extract.Ny, d->extract.Nz),
                 "tsdf_mesh: dims too large for an int32 face count (Nx*Ny*Nz <= %lld)", kTsdfMeshMaxVoxels);
    S2M2_REQUIRE(d->extract.workspace != nullptr, "tsdf_mesh: null workspace (s2m2_tsdf_mesh_workspace_bytes)");
    S2M2_REQUIRE(((uintptr_t)d->extract.workspace & 3) == 0, "tsdf_mesh: the workspace must be 4-byte aligned");

    char* ws = static_cast<char*>(d->extract.workspace);
    m.x.tile_counts = reinterpret_cast<int*>(ws);
    m.face_tile_counts = m.x.tile_counts + m.x.tiles;
    m.rank_map = reinterpret_cast<int*>(ws + tsdf_mesh_counts_bytes(m.x.n));
    m.faces = static_cast<int*>(d->faces);
    m.face_count = d->face_count;
    m.face_capacity = d->face_capacity;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(m.x.tiles), block(kRasterThreads);
    if (int rc = launch<tsdf_mesh_count_kernel>("tsdf_mesh (count)", grid, block, 0, s, m)) return rc;
    if (int rc = launch<tsdf_mesh_points_kernel>("tsdf_mesh (points)", grid, block, 0, s, m)) return rc;
    return launch<tsdf_mesh_faces_kernel>("tsdf_mesh (faces)", grid, block, 0, s, m);
}

}  // namespace s2m2

extern "C" size_t s2m2_tsdf_mesh_workspace_bytes(int Nx, int Ny, int Nz) {
    using namespace s2m2;
    if (!tsdf_mesh_dims_ok(Nx, Ny, Nz)) return 0;
    const long long n = (long long)Nx * Ny * Nz;
    return tsdf_mesh_counts_bytes(n) + round256((size_t)n * sizeof(int));
}

extern "C" int s2m2_tsdf_mesh(const s2m2_tsdf_mesh_desc* desc, void* stream) { return s2m2::tsdf_mesh_impl(desc, stream); }
