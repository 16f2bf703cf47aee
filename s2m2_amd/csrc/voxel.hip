// K23: voxel-grid downsampling of K15's point cloud (include/s2m2_hip.h: s2m2_voxel) -- one record per occupied voxel, the centroid and the mean
// colour of the kept points in it, in the raster order of every voxel's first point.  Four launches (five with `index`), no host step, no
// launch count that depends on the data, no block that waits for another:
//   voxel_clear_kernel    the pair's hash table (keys empty, sums 0, first = INT_MAX) and its counters
//   voxel_insert_kernel   K15's tile walk: keep, z, x, y and the colour bytes by cloud_device.h's functions, the quantisation, then per run of
//                         equal consecutive keys ONE insertion (64-bit compare-and-swap on the key, linear probing) and one set of integer
//                         atomics (adds for n and the six sums, a minimum for first); the slot of every pixel into an int32 plane
//   voxel_count_kernel    leaders (pixels whose raster index is their voxel's first) per raster tile
//   voxel_rank_kernel     tile prefix + raster_rank_step over the leaders: the records, the weights, count and stats
//   voxel_index_kernel    the record rank of every pixel's voxel (the rank launch left it in the slot's key word)
//
// REPRODUCIBILITY.  Which slot a voxel lands in, and in which order the points of a voxel arrive, depend on the schedule; nothing that is stored
// does.  Every aggregate of a voxel is an integer sum or an integer minimum over its points, and both are independent of the order and of the
// grouping of their operands: n, the sums of the local offsets and of the colour bytes, and first.  The record is a function of the aggregates
// alone, a pixel is its voxel's leader by comparing its own raster index with first, and the rank of a leader is its raster rank among the
// leaders.  Slots appear only as addresses.  Run combining (below) only changes the grouping of the same integer operands.
//
// THE CAP.  A new voxel is claimed by a compare-and-swap on an empty slot's key; exactly one thread wins a voxel, and only that thread then
// asks the pair's occupancy counter for room.  The counter is kept in shards whose budgets add up to max_voxels and only ever counts up; a
// winner refused by one shard tries the next.  So a winner is refused only when max_voxels OTHER voxels have been granted: a pair with at
// most max_voxels distinct voxels never loses a point, however its threads race.  A refused winner raises the pair's full flag and drops
// its run; its slot keeps the key (the pair's records are unspecified from there on).
// BOUNDED WORK.  While a pair fits, at most max_voxels of its >= 2 * max_voxels slots are claimed: the load stays <= 1/2.  In the overflow
// case a point that meets an empty slot while the full flag is up gives up without claiming, so the slots claimed beyond max_voxels are at
// most the insertions that were past that check when the flag rose.  Every probe loop runs over at most `slots` slots, whatever the load; a
// point that finds neither its key nor room gives up and is counted.  No loop waits for a value another thread has yet to write.
//
// RUN COMBINING (S2M2_VOXEL_COMBINE, default 1; 0 = one insertion per point, the A/B of profiles/voxel/voxelbench.txt).  Neighbouring pixels of
// a row mostly share a voxel.  A thread first folds its four pixels into runs of equal consecutive keys; then the runs that touch a thread's
// ends are folded across the lanes of the wave by a segmented inclusive scan (shuffles): a lane whose four pixels are one run and whose key
// equals the last key of the lane before continues that lane's segment.  The last lane of a segment issues the insertion for all of it; the
// slot travels back over the segment by a second, reverse pass.  Runs never cross a wave, a block step or a row.
#include "cloud_device.h"
#include "launch.h"
#include "plan.h"

#include <limits.h>
#include <math.h>

#include <cmath>

#ifndef S2M2_VOXEL_COMBINE
#define S2M2_VOXEL_COMBINE 1
#endif

namespace s2m2 {

constexpr bool kVoxelCombine = S2M2_VOXEL_COMBINE != 0;
constexpr unsigned long long kVoxelEmpty = ~0ull;        // no key: a key has 63 bits
constexpr int kVoxelSub = 1024;                          // local offsets per voxel and axis
// per pair: [1] the full flag, [2] kept, [3] out of range, [4] dropped for a full table; then the occupancy counter in kVoxelShards shards, one
// per 64 bytes: one counter would take every new voxel's returning atomic through one address, which serialises them
constexpr int kVoxelShards = 32, kVoxelShardStride = 16;
constexpr int kVoxelHeaderInts = 16 + kVoxelShards * kVoxelShardStride;

struct alignas(16) VoxelSlot {
    unsigned long long key;     // kVoxelEmpty, the voxel's key, or (behind the rank launch, low word) the rank of its record
    unsigned n;
    int first;
    unsigned long long sx, sy, sz, sr, sg, sb;
};
static_assert(sizeof(VoxelSlot) == 64, "a slot is half a cache line: one insertion touches one");

// what a run of points adds to its voxel (a wave's run is at most 256 points: 32 bits hold every partial sum)
struct VoxelAgg {
    unsigned n, sx, sy, sz, sr, sg, sb;
    int first;
};

struct VoxelParams {
    CloudParams c;              // the inputs of K15 (its outputs are null) and K15's tile geometry
    VoxelSlot* table;           // (B, slots)
    int* header;                // (B, kVoxelHeaderInts)
    int* tile_counts;           // (B, tiles): leaders per tile
    int* plane;                 // (B, H, W): the slot of every pixel, -1: not kept or dropped
    uint4_t* records;
    int* weights;
    int* count;
    int* index;
    int* stats;
    long long capacity;
    unsigned slot_mask;         // slots - 1
    unsigned max_voxels;
    float q;                    // voxel_size / 1024
    int plane_vec, index_vec;
};

__host__ __device__ inline unsigned long long voxel_key(int ix, int iy, int iz) {
    return ((unsigned long long)(unsigned)(ix + (1 << 20)) << 42) | ((unsigned long long)(unsigned)(iy + (1 << 20)) << 21) |
           (unsigned long long)(unsigned)(iz + (1 << 20));
}

// the home slot of a key: the 64-bit finaliser of MurmurHash3 (public domain), then the low bits
__host__ __device__ inline unsigned voxel_home(unsigned long long k, unsigned slot_mask) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (unsigned)k & slot_mask;
}

// ---------------------------------------------------------------------------------------------------------------- clear

// a thread per 16 bytes of the pair's table
__global__ __launch_bounds__(kRasterThreads) void voxel_clear_kernel(const VoxelParams p) {
    const int b = blockIdx.y;
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < kVoxelHeaderInts; i += kRasterThreads) p.header[b * kVoxelHeaderInts + i] = 0;
    const unsigned long long i = (unsigned long long)blockIdx.x * kRasterThreads + threadIdx.x, n = ((unsigned long long)p.slot_mask + 1) * 4;
    if (i >= n) return;
    const uint4_t head = {0xffffffffu, 0xffffffffu, 0u, (unsigned)INT_MAX}, zero = {0u, 0u, 0u, 0u};
    reinterpret_cast<uint4_t*>(p.table + (size_t)b * ((size_t)p.slot_mask + 1))[i] = (i & 3) == 0 ? head : zero;
}

// ---------------------------------------------------------------------------------------------------------------- insert

__device__ __forceinline__ void agg_add(VoxelAgg& a, const VoxelAgg& o) {
    a.n += o.n; a.sx += o.sx; a.sy += o.sy; a.sz += o.sz; a.sr += o.sr; a.sg += o.sg; a.sb += o.sb;
    a.first = min(a.first, o.first);
}

__device__ __forceinline__ VoxelAgg agg_up(const VoxelAgg& a, int d) {
    VoxelAgg o;
    o.n = __shfl_up(a.n, d, 64); o.sx = __shfl_up(a.sx, d, 64); o.sy = __shfl_up(a.sy, d, 64); o.sz = __shfl_up(a.sz, d, 64);
    o.sr = __shfl_up(a.sr, d, 64); o.sg = __shfl_up(a.sg, d, 64); o.sb = __shfl_up(a.sb, d, 64); o.first = __shfl_up(a.first, d, 64);
    return o;
}

__device__ __forceinline__ unsigned* voxel_shard(int* header, int s) { return reinterpret_cast<unsigned*>(header + 16 + s * kVoxelShardStride); }

// Room for the voxel this thread has just claimed (called once per voxel, by the winner of its slot): false when every shard has granted its
// budget.  Shard s grants max_voxels / kVoxelShards voxels (+ 1 for the first max_voxels % kVoxelShards shards): max_voxels in all.  The
// counters only count up -- a value at or above the budget stays there --, so a refusal by every shard means that max_voxels voxels were
// granted.  At most kVoxelShards turns.
__device__ __forceinline__ bool voxel_grant(const VoxelParams& p, int* header, int first) {
    for (int i = 0; i < kVoxelShards; ++i) {
        const int s = (first + i) & (kVoxelShards - 1);
        const unsigned budget = p.max_voxels / kVoxelShards + ((unsigned)s < p.max_voxels % kVoxelShards ? 1u : 0u);
        unsigned* c = voxel_shard(header, s);
        if (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= budget) continue;      // (monotone: no grant is missed)
        if (atomicAdd(c, 1u) < budget) return true;
    }
    return false;
}

// The slot of the pair's table that holds `key`, claimed if need be, with `a` added to it; -1 and a.n added to `dropped` when the table is
// full (head of the file: at most `slots` probes, no waiting).  first_shard: where this wave starts to ask for room.
__device__ __forceinline__ int voxel_insert(const VoxelParams& p, VoxelSlot* table, int* header, int first_shard, unsigned long long key,
                                            const VoxelAgg& a, int& dropped) {
    int* full = header + 1;
    const unsigned home = voxel_home(key, p.slot_mask);
    int slot = -1;
    for (unsigned i = 0; i <= p.slot_mask; ++i) {
        const unsigned s = (home + i) & p.slot_mask;
        unsigned long long k = __hip_atomic_load(&table[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == kVoxelEmpty) {
            if (__hip_atomic_load(full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
            k = atomicCAS(&table[s].key, kVoxelEmpty, key);
            if (k == kVoxelEmpty) {                          // this thread, and no other, has claimed the voxel
                if (voxel_grant(p, header, first_shard)) slot = (int)s;
                else atomicExch(full, 1);
                break;
            }
        }
        if (k == key) { slot = (int)s; break; }
    }
    if (slot < 0) { dropped += (int)a.n; return -1; }
    VoxelSlot* t = table + slot;
    atomicAdd(&t->n, a.n);
    atomicMin(&t->first, a.first);
    atomicAdd(&t->sx, (unsigned long long)a.sx); atomicAdd(&t->sy, (unsigned long long)a.sy); atomicAdd(&t->sz, (unsigned long long)a.sz);
    atomicAdd(&t->sr, (unsigned long long)a.sr); atomicAdd(&t->sg, (unsigned long long)a.sg); atomicAdd(&t->sb, (unsigned long long)a.sb);
    return slot;
}

// X = rintf(x / q) as an integer, false when out of range (|X| >= 2^30, NaN included)
__device__ __forceinline__ bool voxel_quantise(float x, float q, int& X) {
    const float r = rintf(x / q);
    if (!(fabsf(r) < 1073741824.f)) return false;
    X = (int)r;
    return true;
}

template <bool VEC, typename IT>
__global__ __launch_bounds__(kRasterThreads) void voxel_insert_kernel(const VoxelParams p) {
    __shared__ int red[3][kRasterWaves];
    const CloudParams& c = p.c;
    const int b = blockIdx.y, tile = blockIdx.x, lane = threadIdx.x & 63;
    const IT* img = static_cast<const IT*>(c.image) + (size_t)b * 3 * c.H * c.W;
    const size_t img_plane = (size_t)c.H * c.W;
    VoxelSlot* table = p.table + (size_t)b * ((size_t)p.slot_mask + 1);
    int* header = p.header + b * kVoxelHeaderInts;
    const int first_shard = (blockIdx.x * kRasterWaves + (threadIdx.x >> 6)) & (kVoxelShards - 1);
    int kept = 0, out_of_range = 0, dropped = 0;
    for (RasterWalk w(c, tile, c.H); w.more(); w.next()) {
        const int v = w.v, u0 = w.u0();
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (u0 < c.W) cloud_eval4<VEC>(c, b, v, u0, z);
        unsigned long long key[4];
        VoxelAgg agg[4];
        bool valid[4], end[4];
        int start[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            key[j] = kVoxelEmpty;
            valid[j] = false;
            start[j] = j;
            agg[j] = VoxelAgg{0u, 0u, 0u, 0u, 0u, 0u, 0u, INT_MAX};
            if (!(z[j] > 0.f)) continue;
            ++kept;
            float x, y;
            cloud_xy(c, v, u0 + j, z[j], x, y);
            int X = 0, Y = 0, Z = 0;
            if (!(voxel_quantise(x, p.q, X) && voxel_quantise(y, p.q, Y) && voxel_quantise(z[j], p.q, Z))) { ++out_of_range; continue; }
            unsigned cr, cg, cb;
            cloud_colour<IT>(c, img, img_plane, v, u0 + j, cr, cg, cb);
            key[j] = voxel_key(X >> 10, Y >> 10, Z >> 10);
            agg[j] = VoxelAgg{1u, (unsigned)(X & (kVoxelSub - 1)), (unsigned)(Y & (kVoxelSub - 1)), (unsigned)(Z & (kVoxelSub - 1)), cr, cg, cb, v * c.W + u0 + j};
            valid[j] = true;
        }
        // runs inside the thread: agg[j] = the run's points up to j, start[j] its first pixel, end[j] at its last
        if constexpr (kVoxelCombine) {
#pragma unroll
            for (int j = 1; j < 4; ++j)
                if (valid[j] && key[j] == key[j - 1]) { agg_add(agg[j], agg[j - 1]); start[j] = start[j - 1]; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) end[j] = valid[j] && (!kVoxelCombine || j == 3 || key[j + 1] != key[j]);

        int slot[4] = {-1, -1, -1, -1};                      // at the last pixel of a run: its slot
        int tail = -1;                                       // the slot of the run that holds pixel 3
        if constexpr (kVoxelCombine) {
            // runs across the lanes: this lane's tail run (the one with pixel 3) continues the tail run of the lane before iff this lane is a
            // single run and its key is that run's
            const bool single = valid[3] && start[3] == 0;
            const unsigned long long before = __shfl_up(key[3], 1, 64);
            const bool joins = lane > 0 && valid[0] && key[0] == before;     // pixel 0's run continues the tail run of the lane before
            VoxelAgg seg = agg[3];                           // (the empty sum where pixel 3 is not valid)
            int fresh = !(single && joins);                  // this lane starts a segment
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const VoxelAgg o = agg_up(seg, d);
                const int of = __shfl_up(fresh, d, 64);
                if (lane >= d && !fresh) { agg_add(seg, o); fresh = of; }
            }
            const VoxelAgg carry = agg_up(seg, 1);           // the segment that ends with the lane before
            const bool consumed = __shfl_down((int)joins, 1, 64) != 0 && lane < 63;      // the next lane issues this lane's tail run
            constexpr int kUnknown = -2;
            int head = -1;                                   // the slot of the run that holds pixel 0
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!end[j]) continue;
                VoxelAgg a = agg[j];
                if (j == 3) {
                    if (consumed) continue;
                    a = seg;
                } else if (start[j] == 0 && joins) {
                    agg_add(a, carry);
                }
                slot[j] = voxel_insert(p, table, header, first_shard, key[j], a, dropped);
                if (start[j] == 0) head = slot[j];
            }
            tail = valid[3] ? (consumed ? kUnknown : slot[3]) : -1;
            // the slots of the consumed tail runs: from the head run of the next lane, which is that lane's tail run if it is a single run
            int give = single ? tail : head;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int g = __shfl_down(give, d, 64);
                if (tail == kUnknown && lane + d < 64 && g != kUnknown) {
                    tail = g;
                    if (single) give = g;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (end[j]) slot[j] = voxel_insert(p, table, header, first_shard, key[j], agg[j], dropped);
            tail = slot[3];
        }
        // every pixel takes the slot of its run, from the run's last pixel backwards
        int mine[4], cur = -1;
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            if (end[j]) cur = j == 3 ? tail : slot[j];
            mine[j] = valid[j] ? cur : -1;
        }
        if (u0 < c.W) dense_store4(p.plane, raster_dense_row(c, b, v), u0, c.W, p.plane_vec != 0, mine);
    }
    kept = block_sum_int(kept, red[0]);
    out_of_range = block_sum_int(out_of_range, red[1]);
    dropped = block_sum_int(dropped, red[2]);
    if (threadIdx.x == 0) {
        if (kept) atomicAdd(header + 2, kept);
        if (out_of_range) atomicAdd(header + 3, out_of_range);
        if (dropped) atomicAdd(header + 4, dropped);
    }
}

// ---------------------------------------------------------------------------------------------------------------- count, rank, index

// the slots of this thread's four pixels and whether each pixel is its voxel's leader
__device__ __forceinline__ void voxel_leaders(const VoxelParams& p, const VoxelSlot* table, int b, int v, int u0, int slot[4], bool lead[4]) {
    const CloudParams& c = p.c;
#pragma unroll
    for (int j = 0; j < 4; ++j) { slot[j] = -1; lead[j] = false; }
    if (u0 >= c.W) return;
    dense_load4(p.plane, raster_dense_row(c, b, v), u0, c.W, p.plane_vec != 0, slot);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (u0 + j < 0 || u0 + j >= c.W) slot[j] = -1;
        lead[j] = slot[j] >= 0 && table[slot[j]].first == v * c.W + u0 + j;
    }
}

__global__ __launch_bounds__(kRasterThreads) void voxel_count_kernel(const VoxelParams p) {
    __shared__ int red[kRasterWaves];
    const CloudParams& c = p.c;
    const int b = blockIdx.y, tile = blockIdx.x;
    const VoxelSlot* table = p.table + (size_t)b * ((size_t)p.slot_mask + 1);
    int n = 0;
    for (RasterWalk w(c, tile, c.H); w.more(); w.next()) {
        int slot[4];
        bool lead[4];
        voxel_leaders(p, table, b, w.v, w.u0(), slot, lead);
#pragma unroll
        for (int j = 0; j < 4; ++j) n += lead[j];
    }
    n = block_sum_int(n, red);
    if (threadIdx.x == 0) p.tile_counts[(size_t)b * c.tiles + tile] = n;
}

// the record of a voxel: the centroid in double from the integer sums, in the order the header states, and the rounded mean colour
__device__ __forceinline__ uint4_t voxel_record(const VoxelSlot& t, unsigned long long key, float q) {
    const double n = (double)t.n, dq = (double)q;
    const int ix = (int)((key >> 42) & 0x1fffff) - (1 << 20), iy = (int)((key >> 21) & 0x1fffff) - (1 << 20), iz = (int)(key & 0x1fffff) - (1 << 20);
    const float x = (float)(((double)ix * 1024.0 + (double)t.sx / n) * dq);
    const float y = (float)(((double)iy * 1024.0 + (double)t.sy / n) * dq);
    const float z = (float)(((double)iz * 1024.0 + (double)t.sz / n) * dq);
    const unsigned long long n2 = 2ull * t.n;
    const unsigned cr = (unsigned)((2 * t.sr + t.n) / n2), cg = (unsigned)((2 * t.sg + t.n) / n2), cb = (unsigned)((2 * t.sb + t.n) / n2);
    uint4_t o = {__builtin_bit_cast(unsigned, x), __builtin_bit_cast(unsigned, y), __builtin_bit_cast(unsigned, z),
                 cr | (cg << 8) | (cb << 16) | 0xff000000u};
    return o;
}

__global__ __launch_bounds__(kRasterThreads) void voxel_rank_kernel(const VoxelParams p) {
    __shared__ int red[kRasterWaves];
    __shared__ int wave_n[2][kRasterWaves];
    const CloudParams& c = p.c;
    const int b = blockIdx.y, tile = blockIdx.x;
    VoxelSlot* table = p.table + (size_t)b * ((size_t)p.slot_mask + 1);
    long long base = tile_prefix(p.tile_counts + (size_t)b * c.tiles, tile, red);
    uint4_t* rec = p.records + (size_t)b * (size_t)p.capacity;
    int* wt = p.weights + (size_t)b * (size_t)p.capacity;
    int step = 0;
    for (RasterWalk w(c, tile, c.H); w.more(); w.next()) {
        int slot[4];
        bool lead[4];
        voxel_leaders(p, table, b, w.v, w.u0(), slot, lead);
        long long r = raster_rank_step(lead, wave_n, step++, base);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!lead[j]) continue;
            VoxelSlot& t = table[slot[j]];
            if (r < p.capacity) {
                if (p.records) rec[r] = voxel_record(t, t.key, p.q);
                if (p.weights) wt[r] = (int)t.n;
            }
            if (p.index) *reinterpret_cast<int*>(&t.key) = (int)r;         // the key has done its work: the index launch reads the rank here
            ++r;
        }
    }
    if (tile == c.tiles - 1 && threadIdx.x == 0) {
        if (p.count) p.count[b] = (int)base;
        if (p.stats) {
            const int* h = p.header + b * kVoxelHeaderInts;
            p.stats[b * 4 + 0] = h[2]; p.stats[b * 4 + 1] = h[3]; p.stats[b * 4 + 2] = h[4]; p.stats[b * 4 + 3] = (int)base;
        }
    }
}

__global__ __launch_bounds__(kRasterThreads) void voxel_index_kernel(const VoxelParams p) {
    const CloudParams& c = p.c;
    const int b = blockIdx.y, tile = blockIdx.x;
    const VoxelSlot* table = p.table + (size_t)b * ((size_t)p.slot_mask + 1);
    for (RasterWalk w(c, tile, c.H); w.more(); w.next()) {
        const int v = w.v, u0 = w.u0();
        if (u0 >= c.W) continue;
        int slot[4] = {-1, -1, -1, -1}, rank[4];
        const size_t row = raster_dense_row(c, b, v);
        dense_load4(p.plane, row, u0, c.W, p.plane_vec != 0, slot);
#pragma unroll
        for (int j = 0; j < 4; ++j) rank[j] = (u0 + j >= 0 && u0 + j < c.W && slot[j] >= 0) ? *reinterpret_cast<const int*>(&table[slot[j]].key) : -1;
        dense_store4(p.index, row, u0, c.W, p.index_vec != 0, rank);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host

// the slots of a pair's table: the smallest power of two >= 2 * max_voxels; 0 when that would reach 2^31
static long long voxel_slots(long long max_voxels) {
    if (max_voxels < 1 || max_voxels > (1LL << 29)) return 0;
    long long s = 2;
    while (s < 2 * max_voxels) s <<= 1;
    return s;
}

struct VoxelLayout {
    size_t header, tile_counts, plane, table, total;
};

static VoxelLayout voxel_layout(int B, int H, int W, long long slots) {
    VoxelLayout l;
    l.header = 0;
    l.tile_counts = round256((size_t)B * kVoxelHeaderInts * sizeof(int));
    l.plane = l.tile_counts + round256((size_t)B * tiles(H, tile_rows(W, kCloudTilePixels)) * sizeof(int));
    l.table = l.plane + round256((size_t)B * H * W * sizeof(int));
    l.total = l.table + (size_t)B * (size_t)slots * sizeof(VoxelSlot);
    return l;
}

static int voxel_impl(const s2m2_voxel_desc* d, void* stream) {
    S2M2_REQUIRE(d != nullptr, "voxel: null descriptor");
    if (int rc = refuse_while_recording("voxel")) return rc;
    VoxelParams p;
    bool vec = false;
    s2m2_cloud_desc in = d->cloud;                  // the inputs alone: the output fields of the embedded descriptor are ignored
    in.depth = nullptr; in.mask = nullptr; in.records = nullptr; in.count = nullptr; in.workspace = nullptr; in.capacity = 0;
    if (int rc = cloud_validate(&in, "voxel", kCloudTilePixels, p.c, vec, false)) return rc;
    S2M2_REQUIRE(in.image != nullptr, "voxel: null pointer (image)");
    const float vs = (float)d->voxel_size;
    S2M2_REQUIRE(std::isfinite(d->voxel_size) && std::isfinite(vs) && vs > 0.f, "voxel: voxel_size must be finite and > 0 in fp32, got %g", d->voxel_size);
    const long long slots = voxel_slots(d->max_voxels);
    S2M2_REQUIRE(slots > 0, "voxel: max_voxels must be 1..2^29 (the table has 2 * max_voxels slots rounded up to a power of two, below 2^31), got %lld",
                 d->max_voxels);
    S2M2_REQUIRE(d->records || d->weights || d->count || d->index || d->stats,
                 "voxel: no output requested (records, weights, count, index and stats are all null pointers)");
    S2M2_REQUIRE(d->capacity >= 0, "voxel: negative capacity %lld", d->capacity);
    S2M2_REQUIRE(d->capacity == 0 || d->records || d->weights, "voxel: null pointers (records and weights) with capacity %lld", d->capacity);
    S2M2_REQUIRE(((uintptr_t)d->records & 15) == 0, "voxel: records must be 16-byte aligned");
    S2M2_REQUIRE(d->workspace != nullptr, "voxel: null workspace (s2m2_voxel_workspace_bytes)");
    S2M2_REQUIRE(((uintptr_t)d->workspace & 15) == 0, "voxel: the workspace must be 16-byte aligned");
    S2M2_REQUIRE((((uintptr_t)d->weights | (uintptr_t)d->count | (uintptr_t)d->index | (uintptr_t)d->stats) & 3) == 0,
                 "voxel: weights, count, index and stats must be 4-byte aligned");

    const VoxelLayout l = voxel_layout(in.B, in.H, in.W, slots);
    char* ws = static_cast<char*>(d->workspace);
    p.header = reinterpret_cast<int*>(ws + l.header);
    p.tile_counts = reinterpret_cast<int*>(ws + l.tile_counts);
    p.plane = reinterpret_cast<int*>(ws + l.plane);
    p.table = reinterpret_cast<VoxelSlot*>(ws + l.table);
    p.records = d->capacity > 0 ? static_cast<uint4_t*>(d->records) : nullptr;
    p.weights = d->capacity > 0 ? d->weights : nullptr;
    p.count = d->count; p.index = d->index; p.stats = d->stats;
    p.capacity = d->capacity;
    p.slot_mask = (unsigned)(slots - 1);
    p.max_voxels = (unsigned)d->max_voxels;
    p.q = vs / 1024.0f;
    S2M2_REQUIRE(p.q > 0.f, "voxel: voxel_size %g is too small (voxel_size / 1024 is 0 in fp32)", d->voxel_size);
    p.plane_vec = 1;                                         // (the workspace is 16-byte aligned and its pieces are whole 256 bytes)
    p.index_vec = ((uintptr_t)d->index & 15) == 0;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 block(kRasterThreads), grid(p.c.tiles, in.B);
    const dim3 grid_clear((unsigned)((slots * 4 + kRasterThreads - 1) / kRasterThreads), in.B);
    if (int rc = launch<voxel_clear_kernel>("voxel (clear)", grid_clear, block, 0, s, p)) return rc;
    if (int rc = by_image_dtype(in.image_dtype, "voxel", [&](auto ti) {
            using IT = decltype(ti);
            if (vec) return launch<voxel_insert_kernel<true, IT>>("voxel (insert)", grid, block, 0, s, p);
            return launch<voxel_insert_kernel<false, IT>>("voxel (insert)", grid, block, 0, s, p);
        }))
        return rc;
    if (int rc = launch<voxel_count_kernel>("voxel (count)", grid, block, 0, s, p)) return rc;
    if (int rc = launch<voxel_rank_kernel>("voxel (rank)", grid, block, 0, s, p)) return rc;
    if (!d->index) return 0;
    return launch<voxel_index_kernel>("voxel (index)", grid, block, 0, s, p);
}

}  // namespace s2m2

extern "C" size_t s2m2_voxel_workspace_bytes(int B, int H, int W, long long max_voxels) {
    using namespace s2m2;
    const long long slots = voxel_slots(max_voxels);
    if (!raster_extents_ok(B, H, W) || slots == 0) return 0;
    return voxel_layout(B, H, W, slots).total;
}

extern "C" int s2m2_voxel_tile_rows(int H, int W) {
    using namespace s2m2;
    if (!raster_extents_ok(1, H, W)) return 0;
    const int rows = tile_rows(W, kCloudTilePixels);
    return H < rows ? H : rows;
}

extern "C" long long s2m2_voxel_home_slot(int ix, int iy, int iz, long long slots) {
    const int lim = 1 << 20;
    if (slots < 2 || slots > (1LL << 30) || (slots & (slots - 1)) != 0) return -1;
    if (ix < -lim || ix >= lim || iy < -lim || iy >= lim || iz < -lim || iz >= lim) return -1;
    return (long long)s2m2::voxel_home(s2m2::voxel_key(ix, iy, iz), (unsigned)(slots - 1));
}

extern "C" int s2m2_voxel(const s2m2_voxel_desc* desc, void* stream) { return s2m2::voxel_impl(desc, stream); }
