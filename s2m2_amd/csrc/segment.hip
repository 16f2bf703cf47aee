// K22: connected components and speckle filter (include/s2m2_hip.h: s2m2_segment) -- the transitive closure of K20's "joined" relation over the
// 4-neighbourhood of the kept pixels, the size of every component, and the disparity map with the components below min_size removed.  Block
// union-find in four launches (three where the image is one tile), no host step, no launch count that depends on the data, no block that waits
// for another:
//   segment_local_kernel    a block takes a tile of kSegTileRows x kSegTileCols pixels: keep (cloud_device.h: cloud_z) and d into LDS, the tile's
//                           components by union-find in LDS, then every pixel's root as a GLOBAL raster index into parent (-1: not kept) and,
//                           at every root of the tile, the number of its pixels in the tile into sizes (0 elsewhere); zeroes the pair's stats
//   segment_border_kernel   a thread per pixel of a tile's right column / bottom row: the union with its joined neighbour across the border, on
//                           the global parent array
//   segment_flatten_kernel  parent[i] = find(i); a tile's root that is not the component's adds its count to sizes[root]: one atomic per tile and
//                           component, not per pixel (per pixel, the adds of a large component queue on one address: profiles/segment/)
//   segment_output_kernel   a walk over the PADDED geometry: label, size[label], mask, disp_out (with its -1 border) and the four counts
//
// THE INVARIANT.  parent[i] <= i at all times (LDS labels in launch A, the global array afterwards), and a link is only ever LOWERED, by an
// atomic minimum, to a smaller index of the same component.  From it:
//   find    x = parent[x] until parent[x] == x: every step strictly descends, so it ends after at most x steps whatever other threads do to
//           the array meanwhile (every value a slot ever holds is an ancestor-or-self of the slot, below or at it).
//   unite   while (a != b) { if (a < b) swap(a, b); old = atomicMin(&parent[a], b); if (old == a) break; a = old; }
//           a > b at the atomic.  old == a: a was a root and now hangs under b: done.  Otherwise a already hung under old < a; the slot now
//           holds min(old, b), and what is left to unite is old with b, both below a: max(a, b) strictly decreases, so the loop ends after at
//           most max(a, b) turns.  No turn waits for a value that another thread has yet to write.
//   result  links only go to smaller indices of the same component, and every joined edge is united (inside a tile by launch A, across
//           tiles by launch B, or it is implied by three united edges: the column links of segment_local_kernel), so after launch B the
//           root of a component is its smallest raster index whatever the order of arrival; the sizes are integer sums.  The outputs are
//           bit-reproducible.
// Every loop below is one of these two, a fixed-trip loop, or a grid-independent walk.
#include "cloud_device.h"
#include "launch.h"
#include "plan.h"

#include <math.h>

namespace s2m2 {

// The tile of launch A.  64 columns: sixteen 4-pixel groups (raster_tiles.h), one row of a tile per 16 threads.  Rows: 16, 32 or 64
// (profiles/segment/tile_size.txt); LDS is 8 bytes per pixel.
#ifndef S2M2_SEGMENT_TILE_ROWS
#define S2M2_SEGMENT_TILE_ROWS 32
#endif
constexpr int kSegTileRows = S2M2_SEGMENT_TILE_ROWS, kSegTileCols = 64;
constexpr int kSegTilePixels = kSegTileRows * kSegTileCols;
constexpr int kSegRowsPerPass = kRasterThreads * 4 / kSegTileCols;           // 16
constexpr int kSegPasses = kSegTileRows / kSegRowsPerPass;
static_assert(kSegTileRows % kSegRowsPerPass == 0 && kSegPasses >= 1, "a tile is whole passes of the block");

struct SegmentParams {
    CloudParams c;              // the inputs of K15 (its outputs are null; its tile geometry is not used)
    int* parent;                // (B, H, W) in the workspace
    int* sizes;                 // (B, H, W) in the workspace: behind launch A pixels per tile-local component at its tile root, 0 elsewhere; behind
                                // launch C pixels per component at its root (other slots: not read)
    int* label;
    int* size;
    unsigned char* mask;
    float* disp_out;
    int* stats;
    int tiles_x, tiles_y;       // tiles of one pair; tile column tx spans the image columns [tx * kSegTileCols - shift, ...)
    int shift;                  // ox & 3: a 4-pixel group starts at a map column that is a multiple of four (raster_tiles.h)
    int min_size;
    float max_jump;
    int ws_vec, label_vec, size_vec, mask_vec, out_vec;     // 16-byte (mask: 4-byte) aligned bases: dense_load4 / dense_store4 may move a group whole
};

__device__ __forceinline__ bool segment_close(float a, float b, float max_jump) { return fabsf(a - b) <= max_jump; }

// ---------------------------------------------------------------------------------------------------------------- (A) local pass

__device__ __forceinline__ int lds_get(const int* lab, int i) { return __hip_atomic_load(lab + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// find on the tile's labels (head of the file: at most x steps)
__device__ __forceinline__ int lds_find(const int* lab, int x) {
    for (int p = lds_get(lab, x); p != x; p = lds_get(lab, x)) x = p;
    return x;
}

// unite on the tile's labels (head of the file: at most max(a, b) turns)
__device__ __forceinline__ void lds_unite(int* lab, int a, int b) {
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(lab + a, b);
        if (old == a) break;
        a = old;
    }
}

template <bool VEC>
__global__ __launch_bounds__(kRasterThreads) void segment_local_kernel(const SegmentParams p) {
    __shared__ float ds[kSegTilePixels];
    __shared__ int lab[kSegTilePixels];                      // local index of an ancestor-or-self, -1: not kept
    const CloudParams& c = p.c;
    const int b = blockIdx.y, ty = blockIdx.x / p.tiles_x, tx = blockIdx.x - ty * p.tiles_x;
    const int gx = threadIdx.x & 15, gy = threadIdx.x >> 4;
    const int v0 = ty * kSegTileRows, c0 = tx * kSegTileCols - p.shift;      // the tile's first image row and column (c0 may be < 0)
    const int u0 = c0 + gx * 4;                                              // this thread's group, in every pass
    const float mj = p.max_jump;
    if (blockIdx.x == 0 && threadIdx.x < 4 && p.stats) p.stats[b * 4 + threadIdx.x] = 0;

    // keep and d of the tile
    bool k[kSegPasses][4];
    float d[kSegPasses][4];
#pragma unroll
    for (int q = 0; q < kSegPasses; ++q) {
        const int r = q * kSegRowsPerPass + gy, v = v0 + r;
        float z[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) d[q][j] = 0.f;
        if (v < c.H && u0 < c.W) cloud_eval4d<VEC>(c, b, v, u0, z, d[q]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            k[q][j] = z[j] > 0.f;
            ds[r * kSegTileCols + gx * 4 + j] = d[q][j];
            lab[r * kSegTileCols + gx * 4 + j] = k[q][j] ? 0 : -1;             // (>= 0: kept; the links follow behind the barrier)
        }
    }
    __syncthreads();

    // row links: a pixel joined with its left neighbour hangs under it -- inside the group under the first pixel of its run
    bool left[kSegPasses][4];
#pragma unroll
    for (int q = 0; q < kSegPasses; ++q) {
        const int i0 = (q * kSegRowsPerPass + gy) * kSegTileCols + gx * 4;
        left[q][0] = gx > 0 && k[q][0] && lab[i0 - 1] >= 0 && segment_close(d[q][0], ds[i0 - 1], mj);
#pragma unroll
        for (int j = 1; j < 4; ++j) left[q][j] = k[q][j] && k[q][j - 1] && segment_close(d[q][j], d[q][j - 1], mj);
    }
    __syncthreads();                                         // every lab[i0 - 1] >= 0 test is done before the links overwrite the zeros
#pragma unroll
    for (int q = 0; q < kSegPasses; ++q) {
        const int i0 = (q * kSegRowsPerPass + gy) * kSegTileCols + gx * 4;
        int head = i0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!left[q][j]) head = i0 + j;
            else if (j == 0) head = i0 - 1;
            if (k[q][j]) lab[i0 + j] = head;
        }
    }
    __syncthreads();

    // column links.  The union with the pixel above is left out where three united edges imply it: left, the left pixel's own column link,
    // and the row link of the two pixels above (induction along the row: the leftmost pixel of such a chain unites for itself)
#pragma unroll
    for (int q = 0; q < kSegPasses; ++q) {
        const int r = q * kSegRowsPerPass + gy;
        if (r == 0) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = r * kSegTileCols + gx * 4 + j, up = i - kSegTileCols;
            if (!(k[q][j] && lds_get(lab, up) >= 0 && segment_close(d[q][j], ds[up], mj))) continue;
            const bool implied = left[q][j] && lds_get(lab, up - 1) >= 0 && segment_close(ds[i - 1], ds[up - 1], mj) && segment_close(ds[up - 1], ds[up], mj);
            if (!implied) lds_unite(lab, lds_find(lab, i), lds_find(lab, up));
        }
    }
    __syncthreads();

    // the pixels of every root: d is no longer needed, its LDS holds the counts.  A thread's run of pixels with one root adds once
    int* cnt = reinterpret_cast<int*>(ds);
    int root[kSegPasses][4];
#pragma unroll
    for (int q = 0; q < kSegPasses; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = (q * kSegRowsPerPass + gy) * kSegTileCols + gx * 4 + j;
            root[q][j] = k[q][j] ? lds_find(lab, i) : -1;
            cnt[i] = 0;
        }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kSegPasses; ++q) {
        int run = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (root[q][j] >= 0) ++run;
            if (run && (j == 3 || root[q][j + 1] != root[q][j])) {
                atomicAdd(cnt + root[q][j], run);
                run = 0;
            }
        }
    }
    __syncthreads();

    // roots as global raster indices, counts at the roots
#pragma unroll
    for (int q = 0; q < kSegPasses; ++q) {
        const int r = q * kSegRowsPerPass + gy, v = v0 + r;
        if (!(v < c.H && u0 < c.W)) continue;
        int par[4], num[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = r * kSegTileCols + gx * 4 + j;
            par[j] = root[q][j] < 0 ? -1 : (v0 + root[q][j] / kSegTileCols) * c.W + (c0 + root[q][j] % kSegTileCols);
            num[j] = root[q][j] == i ? cnt[i] : 0;
        }
        const size_t row = raster_dense_row(c, b, v);
        dense_store4(p.parent, row, u0, c.W, p.ws_vec != 0, par);
        dense_store4(p.sizes, row, u0, c.W, p.ws_vec != 0, num);
    }
}

// ---------------------------------------------------------------------------------------------------------------- (B) border merge

// a load that another CU's atomics may have changed since this CU last read the line: served by L2, not by a stale L1 line
__device__ __forceinline__ int global_get(const int* parent, int i) { return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int global_find(const int* parent, int x) {
    for (int q = global_get(parent, x); q != x; q = global_get(parent, x)) x = q;
    return x;
}

__device__ __forceinline__ void global_unite(int* parent, int a, int b) {
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);
        if (old == a) break;
        a = old;
    }
}

// Threads [0, nvb * H): vertical borders, thread -> (border k, row v): pixel (v, u) with its right neighbour, u = (k + 1) * kSegTileCols - shift - 1.
// Threads behind them: horizontal borders, thread -> (border k, column u): pixel (v, u) with the one below, v = (k + 1) * kSegTileRows - 1.
__global__ __launch_bounds__(kRasterThreads) void segment_border_kernel(const SegmentParams p, int n_vertical, int n_total) {
    const CloudParams& c = p.c;
    const int b = blockIdx.y;
    const long long tl = (long long)blockIdx.x * kRasterThreads + threadIdx.x;
    if (tl >= n_total) return;
    int t = (int)tl, v, u, v1, u1;
    const bool vertical = t < n_vertical;
    if (vertical) {
        const int kb = t / c.H;
        v = t - kb * c.H; u = (kb + 1) * kSegTileCols - p.shift - 1;
        v1 = v; u1 = u + 1;
    } else {
        t -= n_vertical;
        const int kb = t / c.W;
        u = t - kb * c.W; v = (kb + 1) * kSegTileRows - 1;
        v1 = v + 1; u1 = u;
    }
    int* parent = p.parent + (size_t)b * c.H * c.W;
    const int i = v * c.W + u, i1 = v1 * c.W + u1;
    if (parent[i] < 0 || parent[i1] < 0) return;             // the sign of a slot never changes: a plain load will do
    const float d0 = c.disp[raster_map_index(c, b, v, u)], d1 = c.disp[raster_map_index(c, b, v1, u1)];
    if (!segment_close(d0, d1, p.max_jump)) return;
    // As in launch A, the union is left out where three united edges imply it: the same border edge one pixel back along the border (one row
    // up / one column left) and the two edges that lead there.  The dependencies must not run in a circle.  A vertical border's edge in a row
    // that is not the first of its tile leans on in-tile column edges (launch A) and on the border edge of the row above alone; a horizontal
    // border's edge leans on the one left of it and on row edges, which are in-tile or vertical-border edges.  Only the first row of a tile
    // would lean on horizontal-border edges in turn (the four edges round a tile corner): there the union is always made.
    if (vertical ? v % kSegTileRows != 0 : u > 0) {
        const int pv = vertical ? v - 1 : v, pu = vertical ? u : u - 1, pv1 = vertical ? v1 - 1 : v1, pu1 = vertical ? u1 : u1 - 1;
        if (parent[pv * c.W + pu] >= 0 && parent[pv1 * c.W + pu1] >= 0) {
            const float e0 = c.disp[raster_map_index(c, b, pv, pu)], e1 = c.disp[raster_map_index(c, b, pv1, pu1)];
            if (segment_close(e0, d0, p.max_jump) && segment_close(e1, d1, p.max_jump) && segment_close(e0, e1, p.max_jump)) return;
        }
    }
    global_unite(parent, global_find(parent, i), global_find(parent, i1));
}

// ---------------------------------------------------------------------------------------------------------------- (C) flatten

__global__ __launch_bounds__(kRasterThreads) void segment_flatten_kernel(const SegmentParams p, int n) {
    const int b = blockIdx.y;
    const long long il = (long long)blockIdx.x * kRasterThreads + threadIdx.x;
    if (il >= n) return;
    const int i = (int)il;
    int* parent = p.parent + (size_t)b * n;
    int* sizes = p.sizes + (size_t)b * n;
    if (parent[i] < 0) return;
    const int root = global_find(parent, i);
    parent[i] = root;                                        // a slot that other threads walk through: the root is an ancestor like any other
    // a tile's root that hangs under another: its count moves to the component's root.  Nothing adds to sizes[i] here (only final roots
    // receive), and a final root keeps its own tile's count as the start of the sum
    const int mine = sizes[i];
    if (mine > 0 && root != i) atomicAdd(sizes + root, mine);
}

// ---------------------------------------------------------------------------------------------------------------- (D) outputs

// a thread takes four consecutive columns of one PADDED row: up0 = 4 * group, so the image column u0 = up0 - ox puts a group at a map column
// that is a multiple of four, as raster_tiles.h does
template <bool VEC>
__global__ __launch_bounds__(kRasterThreads) void segment_output_kernel(const SegmentParams p, int groups_per_row, long long n_groups) {
    __shared__ int red[4][kRasterWaves];
    const CloudParams& c = p.c;
    const int b = blockIdx.y;
    const long long g = (long long)blockIdx.x * kRasterThreads + threadIdx.x;
    int kept = 0, comps = 0, surv = 0, surv_comps = 0;
    if (g < n_groups) {
        const int vp = (int)(g / groups_per_row), up0 = (int)(g - (long long)vp * groups_per_row) * 4;
        const int v = vp - c.oy, u0 = up0 - c.ox;
        const bool in_row = v >= 0 && v < c.H && u0 + 3 >= 0 && u0 < c.W;
        int lab[4] = {-1, -1, -1, -1}, sz[4] = {0, 0, 0, 0};
        unsigned char m[4] = {0, 0, 0, 0};
        if (in_row) {
            const size_t row = raster_dense_row(c, b, v);
            dense_load4(p.parent, row, u0, c.W, p.ws_vec != 0, lab);
            const int* sizes = p.sizes + (size_t)b * c.H * c.W;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (lab[j] < 0) continue;
                sz[j] = sizes[lab[j]];
                m[j] = sz[j] >= p.min_size;
                kept += 1;
                surv += m[j];
                if (lab[j] == v * c.W + u0 + j) { comps += 1; surv_comps += m[j]; }
            }
            if (p.label) dense_store4(p.label, row, u0, c.W, p.label_vec != 0, lab);
            if (p.size) dense_store4(p.size, row, u0, c.W, p.size_vec != 0, sz);
            if (p.mask) dense_store4(p.mask, row, u0, c.W, p.mask_vec != 0, m);
        }
        if (p.disp_out) {
            const size_t mi = ((size_t)b * c.Hp + vp) * (size_t)c.Wp + up0;
            float o[4] = {-1.f, -1.f, -1.f, -1.f};
            if (in_row) {
                float dv[4];
                map_load4<VEC>(c.disp, mi, u0, c.W, dv);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (m[j]) o[j] = dv[j];
            }
            if constexpr (VEC) {
                typedef float float4_t __attribute__((ext_vector_type(4)));
                const float4_t ov = {o[0], o[1], o[2], o[3]};
                *reinterpret_cast<float4_t*>(p.disp_out + mi) = ov;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (up0 + j < c.Wp) p.disp_out[mi + j] = o[j];
            }
        }
    }
    if (p.stats) {                                           // block sums, then one atomic per count and block (block-uniform branch)
        kept = block_sum_int(kept, red[0]);
        comps = block_sum_int(comps, red[1]);
        surv = block_sum_int(surv, red[2]);
        surv_comps = block_sum_int(surv_comps, red[3]);
        if (threadIdx.x == 0) {
            if (kept) atomicAdd(p.stats + b * 4 + 0, kept);
            if (comps) atomicAdd(p.stats + b * 4 + 1, comps);
            if (surv) atomicAdd(p.stats + b * 4 + 2, surv);
            if (surv_comps) atomicAdd(p.stats + b * 4 + 3, surv_comps);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host

// raster indices, sizes and the counts are int32, and a size is compared with min_size <= 2^30
static bool segment_extents_ok(int B, int H, int W) { return raster_extents_ok(B, H, W, 1LL << 30); }

static size_t segment_plane_bytes(int B, int H, int W) { return round256((size_t)B * H * W * sizeof(int)); }

static int segment_impl(const s2m2_segment_desc* d, void* stream) {
    S2M2_REQUIRE(d != nullptr, "segment: null descriptor");
    if (int rc = refuse_while_recording("segment")) return rc;
    SegmentParams p;
    bool vec = false;
    s2m2_cloud_desc in = d->cloud;                  // the inputs alone: the output fields of the embedded descriptor are ignored
    in.depth = nullptr; in.mask = nullptr; in.records = nullptr; in.count = nullptr; in.workspace = nullptr; in.capacity = 0;
    if (int rc = cloud_validate(&in, "segment", kCloudTilePixels, p.c, vec, false)) return rc;
    S2M2_REQUIRE(segment_extents_ok(in.B, in.H, in.W), "segment: extents too large (H*W < 2^30)");
    S2M2_REQUIRE(d->label || d->size || d->mask || d->disp_out || d->stats,
                 "segment: no output requested (label, size, mask, disp_out and stats are all null pointers)");
    S2M2_REQUIRE(d->workspace != nullptr, "segment: null workspace (s2m2_segment_workspace_bytes)");
    S2M2_REQUIRE(((uintptr_t)d->workspace & 3) == 0, "segment: the workspace must be 4-byte aligned");
    S2M2_REQUIRE((((uintptr_t)d->label | (uintptr_t)d->size | (uintptr_t)d->disp_out | (uintptr_t)d->stats) & 3) == 0,
                 "segment: label, size, disp_out and stats must be 4-byte aligned");
    S2M2_REQUIRE(d->disp_out != in.disp, "segment: disp_out aliases cloud.disp");
    S2M2_REQUIRE(d->max_jump >= 0.0, "segment: max_jump must be >= 0 (+inf is allowed), got %g", d->max_jump);       // false for NaN
    S2M2_REQUIRE(d->min_size >= 1 && d->min_size <= (1LL << 30), "segment: min_size must be 1..2^30 (%lld)", d->min_size);

    const CloudParams& c = p.c;
    const int n = in.H * in.W;
    p.parent = static_cast<int*>(d->workspace);
    p.sizes = reinterpret_cast<int*>(static_cast<char*>(d->workspace) + segment_plane_bytes(in.B, in.H, in.W));
    p.label = d->label; p.size = d->size; p.mask = d->mask; p.disp_out = d->disp_out; p.stats = d->stats;
    p.shift = c.ox & 3;
    p.tiles_x = (int)(((long long)in.W + p.shift + kSegTileCols - 1) / kSegTileCols);
    p.tiles_y = tiles(in.H, kSegTileRows);
    p.min_size = (int)d->min_size;
    p.max_jump = (float)d->max_jump;
    p.ws_vec = ((uintptr_t)d->workspace & 15) == 0;          // (both planes: the first is whole 256-byte pieces)
    p.label_vec = ((uintptr_t)d->label & 15) == 0;
    p.size_vec = ((uintptr_t)d->size & 15) == 0;
    p.mask_vec = ((uintptr_t)d->mask & 3) == 0;
    const bool out_vec = vec && ((uintptr_t)d->disp_out & 15) == 0;
    p.out_vec = out_vec;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 block(kRasterThreads);
    const dim3 grid_a((unsigned)((long long)p.tiles_x * p.tiles_y), in.B);
    if (int rc = vec ? launch<segment_local_kernel<true>>("segment (local)", grid_a, block, 0, s, p)
                     : launch<segment_local_kernel<false>>("segment (local)", grid_a, block, 0, s, p))
        return rc;
    // tile borders with image pixels on both sides: a function of the extents alone
    const int nvb = (int)(((long long)in.W + p.shift - 1) / kSegTileCols), nhb = (in.H - 1) / kSegTileRows;
    const long long n_vertical = (long long)nvb * in.H, n_border = n_vertical + (long long)nhb * in.W;       // < 2 * H * W / 16
    if (n_border > 0) {
        const dim3 grid_b((unsigned)((n_border + kRasterThreads - 1) / kRasterThreads), in.B);
        if (int rc = launch<segment_border_kernel>("segment (border)", grid_b, block, 0, s, p, (int)n_vertical, (int)n_border)) return rc;
    }
    const dim3 grid_c((unsigned)((n + kRasterThreads - 1) / kRasterThreads), in.B);
    if (int rc = launch<segment_flatten_kernel>("segment (flatten)", grid_c, block, 0, s, p, n)) return rc;
    const int groups_per_row = (in.Wp + 3) / 4;
    const long long n_groups = (long long)groups_per_row * in.Hp;
    const dim3 grid_d((unsigned)((n_groups + kRasterThreads - 1) / kRasterThreads), in.B);
    return out_vec ? launch<segment_output_kernel<true>>("segment (outputs)", grid_d, block, 0, s, p, groups_per_row, n_groups)
                   : launch<segment_output_kernel<false>>("segment (outputs)", grid_d, block, 0, s, p, groups_per_row, n_groups);
}

}  // namespace s2m2

extern "C" size_t s2m2_segment_workspace_bytes(int B, int H, int W) {
    if (!s2m2::segment_extents_ok(B, H, W)) return 0;
    return 2 * s2m2::segment_plane_bytes(B, H, W);
}

extern "C" int s2m2_segment_tile_rows(int H, int W) { return s2m2::segment_extents_ok(1, H, W) ? (H < s2m2::kSegTileRows ? H : s2m2::kSegTileRows) : 0; }

extern "C" int s2m2_segment_tile_cols(int H, int W) { return s2m2::segment_extents_ok(1, H, W) ? (W < s2m2::kSegTileCols ? W : s2m2::kSegTileCols) : 0; }

extern "C" int s2m2_segment(const s2m2_segment_desc* desc, void* stream) { return s2m2::segment_impl(desc, stream); }
