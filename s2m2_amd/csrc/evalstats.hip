// K18: the evaluation stage behind the forward (include/s2m2_hip.h: s2m2_disp_eval) -- disparity error statistics against ground truth as one
// block of 64-bit integer words per pair.  Two launches without a host step, global atomics or waiting between blocks:
//   eval_tile_kernel   a block owns a tile of whole rows of one pair.  The ALL / KEPT counts are bit fields of two 64-bit registers per thread
//                      (EvalCounters), the four fixed-point sums are 64-bit registers per thread, the histogram and the confidence table
//                      are integer adds in LDS (order independent); the loads of the next step are in flight while a step is counted.
//                      The block stores ONE partial block per tile into the workspace, in a compact form: kEvalPartLo 32-bit words in
//                      the order of the stat block (a tile holds fewer than 2^31 pixels, so every count fits), followed by the high
//                      halves of the words that are sums of q or s and can pass 2^32 inside a tile (kEvalWide of them).
//   eval_sum_kernel    32 words x 32 slices of tiles per block: every thread sums its word over every 32nd tile, the slices meet in LDS, and
//                      every word of the pair's stat block is written.
// In LDS the confidence table is kept as LEVELS: level k = the number of thresholds a pixel's error exceeds (thresholds increase strictly, so
// bad[t] <=> k > t; a non-finite prediction has k = nthr).  One add per pixel stands for the count and all eight bad counters of the row; the
// block turns levels into count / bad[t] when it stores its partial block.
// Pixel -> thread map, map loads and the loads of gt and region (which follow the unpadded rows): raster_tiles.h, shared with K15 and K20.
#include <math.h>

#include "raster_tiles.h"
#include "launch.h"
#include "plan.h"

namespace s2m2 {

typedef unsigned long long u64;

constexpr int kEvalTilePixels = 4096;                    // a tile (raster_host.h: tile_rows_capped) ...
constexpr int kEvalMaxTiles = 1024;                      // ... with more rows where a pair would have more tiles than this (launch B's loop)
constexpr int kEvalLevels = S2M2_EVAL_MAX_THR + 1;
constexpr int kEvalWide = 4 + S2M2_EVAL_CONF_BINS;       // ALL and KEPT: SUM_ABS_Q, SUM_SQ_Q; CONF: SUM_ABS_Q of every row
constexpr int kEvalPartLo = S2M2_EVAL_WORDS;
constexpr int kEvalPart = (kEvalPartLo + kEvalWide + 3) / 4 * 4;         // 32-bit words of one partial block
constexpr int kEvalSumThreads = 1024, kEvalSumWords = 32, kEvalSumSlices = kEvalSumThreads / kEvalSumWords;      // launch B

static_assert(S2M2_EVAL_BLOCK_WORDS == 6 + S2M2_EVAL_MAX_THR && S2M2_EVAL_CONF_ROW_WORDS == 2 + S2M2_EVAL_MAX_THR, "stat block layout");
static_assert(S2M2_EVAL_KEPT == S2M2_EVAL_ALL + S2M2_EVAL_BLOCK_WORDS && S2M2_EVAL_HIST == S2M2_EVAL_KEPT + S2M2_EVAL_BLOCK_WORDS, "stat block layout");
static_assert(S2M2_EVAL_CONF == S2M2_EVAL_HIST + S2M2_EVAL_HIST_BINS, "stat block layout");
static_assert(S2M2_EVAL_WORDS == S2M2_EVAL_CONF + S2M2_EVAL_CONF_BINS * S2M2_EVAL_CONF_ROW_WORDS, "stat block layout");

static inline int eval_tile_rows(int H, int W) { return tile_rows_capped(H, W, kEvalTilePixels, kEvalMaxTiles); }

// index of stat word w among the high halves of a partial block, or -1: the word is a count
__host__ __device__ __forceinline__ int eval_wide_index(int w) {
    if (w == S2M2_EVAL_ALL + S2M2_EVAL_SUM_ABS_Q) return 0;
    if (w == S2M2_EVAL_ALL + S2M2_EVAL_SUM_SQ_Q) return 1;
    if (w == S2M2_EVAL_KEPT + S2M2_EVAL_SUM_ABS_Q) return 2;
    if (w == S2M2_EVAL_KEPT + S2M2_EVAL_SUM_SQ_Q) return 3;
    if (w >= S2M2_EVAL_CONF && (w - S2M2_EVAL_CONF) % S2M2_EVAL_CONF_ROW_WORDS == S2M2_EVAL_CONF_SUM_ABS_Q)
        return 4 + (w - S2M2_EVAL_CONF) / S2M2_EVAL_CONF_ROW_WORDS;
    return -1;
}

struct EvalParams {
    const float* disp;
    const float* occ;
    const float* conf;
    const float* gt;
    const unsigned char* region;
    unsigned* part;             // (B, tiles, kEvalPart)
    int H, W, Hp, Wp;
    int oy, ox;                 // crop offsets
    int rows_per_tile, tiles;   // tiles per pair
    int nthr;
    int gt_vec, region_vec;     // gt is 16-byte aligned / region is 4-byte aligned: aligned groups take one load
    float thr[S2M2_EVAL_MAX_THR];       // slots t >= nthr hold +inf: never exceeded
    float d1_abs, d1_rel, gt_min, conf_min, occ_min;
};

__device__ __forceinline__ bool eval_finite(float x) { return fabsf(x) < INFINITY; }      // false for NaN

// The counters of one set of pixels (ALL or KEPT), per thread and packed so that a pixel costs two 64-bit adds: `levels` holds nine 7-bit
// fields -- field k counts the evaluated pixels whose error exceeds exactly k thresholds, so bad[t] = the fields above t --, `flags` four
// 16-bit fields (in the region, evaluated, not finite, D1).  A 7-bit field holds 127 pixels: flush() at least every kEvalFlushSteps steps.
constexpr int kEvalFlushSteps = 31;                      // x 4 pixels = 124 <= 127
constexpr int kEvalLevelBits = 7;

struct EvalCounters {
    u64 levels = 0, flags = 0, sum_abs_q = 0, sum_sq_q = 0;

    __device__ __forceinline__ void add(bool in_region, bool evaluated, bool finite, bool d1, int level, unsigned q, u64 s) {
        levels += evaluated ? 1ull << (kEvalLevelBits * level) : 0ull;
        flags += (u64)in_region | (u64)evaluated << 16 | (u64)(evaluated && !finite) << 32 | (u64)(evaluated && d1) << 48;
        const bool summed = evaluated && finite;
        sum_abs_q += summed ? q : 0u;
        sum_sq_q += summed ? s : 0ull;
    }

    // Into the block's words (LDS, zeroed) and back to zero: wave sums, then one add per wave and word.  Every lane of the wave calls it.
    // The level fields are widened to 16 bits first: 64 lanes x 127 fits.
    __device__ __forceinline__ void flush(u64* words) {
        u64 wide[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < kEvalLevels; ++k) wide[k >> 2] |= ((levels >> (kEvalLevelBits * k)) & 127u) << (16 * (k & 3));
#pragma unroll
        for (int i = 0; i < 3; ++i) wide[i] = wave_sum_u64(wide[i]);
        const u64 f = wave_sum_u64(flags), sa = wave_sum_u64(sum_abs_q), ss = wave_sum_u64(sum_sq_q);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&words[S2M2_EVAL_N_REGION], f & 0xffffu);
            atomicAdd(&words[S2M2_EVAL_N_EVAL], (f >> 16) & 0xffffu);
            atomicAdd(&words[S2M2_EVAL_N_NONFINITE], (f >> 32) & 0xffffu);
            atomicAdd(&words[S2M2_EVAL_D1_BAD], f >> 48);
            atomicAdd(&words[S2M2_EVAL_SUM_ABS_Q], sa);
            atomicAdd(&words[S2M2_EVAL_SUM_SQ_Q], ss);
            u64 above = 0;                               // pixels of the levels above t
#pragma unroll
            for (int t = S2M2_EVAL_MAX_THR - 1; t >= 0; --t) {
                above += (wide[(t + 1) >> 2] >> (16 * ((t + 1) & 3))) & 0xffffu;
                atomicAdd(&words[S2M2_EVAL_BAD + t], above);
            }
        }
        levels = flags = sum_abs_q = sum_sq_q = 0;
    }
};

// the four pixels of a thread: maps, ground truth, region byte (1 without a region); pixels outside the row keep the zeros
struct EvalPixels {
    float d[4], o[4], c[4], g[4];
    unsigned r[4];
};

// row v of pair b, first column u0 (may be < 0 or reach beyond W)
template <bool VEC, bool CONF>
__device__ __forceinline__ void eval_load(const EvalParams& p, int b, int v, int u0, EvalPixels& x) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { x.d[j] = 0.f; x.o[j] = 0.f; x.c[j] = 0.f; x.g[j] = 0.f; x.r[j] = 1u; }
    if (u0 >= p.W) return;
    const size_t row = raster_dense_row(p, b, v), m = raster_map_index(p, b, v, u0);
    map_load4<VEC>(p.disp, m, u0, p.W, x.d);
    if constexpr (CONF) {
        map_load4<VEC>(p.occ, m, u0, p.W, x.o);
        map_load4<VEC>(p.conf, m, u0, p.W, x.c);
    }
    dense_load4(p.gt, row, u0, p.W, p.gt_vec != 0, x.g);
    if (p.region) {
        unsigned char r[4] = {1, 1, 1, 1};
        dense_load4(p.region, row, u0, p.W, p.region_vec != 0, r);
#pragma unroll
        for (int j = 0; j < 4; ++j) x.r[j] = r[j];
    }
}

template <bool VEC, bool CONF>
__global__ __launch_bounds__(kRasterThreads) void eval_tile_kernel(const EvalParams p) {
    __shared__ unsigned hist[S2M2_EVAL_HIST_BINS];
    __shared__ unsigned levels[S2M2_EVAL_CONF_BINS * kEvalLevels];
    __shared__ u64 conf_sum[S2M2_EVAL_CONF_BINS];
    __shared__ u64 words[2 * S2M2_EVAL_BLOCK_WORDS];         // ALL, KEPT
    const int tid = threadIdx.x;
    for (int i = tid; i < S2M2_EVAL_HIST_BINS; i += kRasterThreads) hist[i] = 0;
    for (int i = tid; i < S2M2_EVAL_CONF_BINS * kEvalLevels; i += kRasterThreads) levels[i] = 0;
    if (tid < S2M2_EVAL_CONF_BINS) conf_sum[tid] = 0;
    if (tid < 2 * S2M2_EVAL_BLOCK_WORDS) words[tid] = 0;
    __syncthreads();

    const int b = blockIdx.y, tile = blockIdx.x;
    // block-uniform steps of kRasterChunk pixels (every lane takes every step: the flushes are whole waves): row by row, left to right
    EvalCounters all, kept;
    EvalPixels cur, next = {};
    RasterWalk w(p, tile, p.H);                             // (a tile has at least one row)
    eval_load<VEC, CONF>(p, b, w.v, w.u0(), cur);
    for (int step = 0; w.more(); ++step) {
        const int u0 = w.u0();
        w.next();
        if (w.more()) eval_load<VEC, CONF>(p, b, w.v, w.u0(), next);         // in flight while this step is counted
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in_region = u0 + j >= 0 && u0 + j < p.W && cur.r[j] != 0;
            const bool evaluated = in_region && eval_finite(cur.g[j]) && cur.g[j] > p.gt_min;
            const bool finite = eval_finite(cur.d[j]);
            const float e = cur.d[j] - cur.g[j], a = fabsf(e);
            int level = 0;
#pragma unroll
            for (int t = 0; t < S2M2_EVAL_MAX_THR; ++t) level += a > p.thr[t];
            if (!finite) level = p.nthr;
            const bool d1 = !finite || (a > p.d1_abs && a > p.d1_rel * fabsf(cur.g[j]));
            // fixed point: only where the pixel is summed, so that no conversion ever sees a NaN
            const bool summed = evaluated && finite;
            const float as = summed ? a : 0.f, es = summed ? e : 0.f;
            const unsigned q = (unsigned)rintf(fminf(as, 1024.f) * 65536.f);               // <= 2^26
            const float sq = fminf(es * es, 1048576.f) * 4096.f;                           // <= 2^32, an integer from 2^24 on
            const u64 s = sq >= 4294967296.f ? (1ull << 32) : (u64)(unsigned)rintf(sq);
            all.add(in_region, evaluated, finite, d1, level, q, s);
            if (summed) {
                const float h = as * 64.f;
                atomicAdd(&hist[h >= 1024.f ? 1024 : (int)h], 1u);
            }
            if constexpr (CONF) {
                const bool keep = cloud_valid(cur.c[j], cur.o[j], p.conf_min, p.occ_min);
                kept.add(in_region && keep, evaluated && keep, finite, d1, level, q, s);
                const float cs = cur.c[j] * 64.f;
                const int cbin = !(cs >= 0.f) ? 0 : (cs >= 63.f ? 63 : (int)cs);          // NaN -> 0
                if (evaluated) atomicAdd(&levels[cbin * kEvalLevels + level], 1u);
                if (summed) atomicAdd(&conf_sum[cbin], (u64)q);
            }
        }
        cur = next;
        if ((step + 1) % kEvalFlushSteps == 0) {          // block-uniform
            all.flush(words);
            if constexpr (CONF) kept.flush(words + S2M2_EVAL_BLOCK_WORDS);
        }
    }
    all.flush(words);
    if constexpr (CONF) kept.flush(words + S2M2_EVAL_BLOCK_WORDS);
    __syncthreads();

    // the partial block of this tile: low halves in the order of the stat block, then the high halves of the wide words
    unsigned* part = p.part + ((size_t)b * p.tiles + tile) * kEvalPart;
    for (int w = tid; w < kEvalPart; w += kRasterThreads) {
        u64 x = 0;
        if (w < S2M2_EVAL_HIST) x = words[w];
        else if (w < S2M2_EVAL_CONF) x = hist[w - S2M2_EVAL_HIST];
        else if (w < S2M2_EVAL_WORDS) {
            const int cbin = (w - S2M2_EVAL_CONF) / S2M2_EVAL_CONF_ROW_WORDS, f = (w - S2M2_EVAL_CONF) % S2M2_EVAL_CONF_ROW_WORDS;
            if (f == S2M2_EVAL_CONF_SUM_ABS_Q) x = conf_sum[cbin];
            else {                                           // COUNT: every level; BAD + t: the levels above t
                const int first = f == S2M2_EVAL_CONF_COUNT ? 0 : f - S2M2_EVAL_CONF_BAD + 1;
                for (int k = first; k < kEvalLevels; ++k) x += levels[cbin * kEvalLevels + k];
            }
        } else if (w < S2M2_EVAL_WORDS + kEvalWide) {
            const int i = w - S2M2_EVAL_WORDS;
            x = (i < 4 ? words[(i >> 1) * S2M2_EVAL_BLOCK_WORDS + S2M2_EVAL_SUM_ABS_Q + (i & 1)] : conf_sum[i - 4]) >> 32;
        }
        part[w] = (unsigned)x;
    }
}

__global__ __launch_bounds__(kEvalSumThreads) void eval_sum_kernel(const unsigned* __restrict__ part, u64* __restrict__ stats, int tiles) {
    __shared__ u64 lo_s[kEvalSumSlices][kEvalSumWords], hi_s[kEvalSumSlices][kEvalSumWords];
    const int b = blockIdx.y, col = threadIdx.x % kEvalSumWords, slice = threadIdx.x / kEvalSumWords;
    const int w = blockIdx.x * kEvalSumWords + col;
    u64 lo = 0, hi = 0;
    if (w < S2M2_EVAL_WORDS) {
        const int wide = eval_wide_index(w);
        const unsigned* base = part + (size_t)b * tiles * kEvalPart;
#pragma unroll 4
        for (int t = slice; t < tiles; t += kEvalSumSlices) {           // independent loads: several in flight
            lo += base[(size_t)t * kEvalPart + w];
            if (wide >= 0) hi += base[(size_t)t * kEvalPart + S2M2_EVAL_WORDS + wide];
        }
    }
    lo_s[slice][col] = lo;
    hi_s[slice][col] = hi;
    __syncthreads();
    if (slice == 0 && w < S2M2_EVAL_WORDS) {
#pragma unroll
        for (int s = 1; s < kEvalSumSlices; ++s) { lo += lo_s[s][col]; hi += hi_s[s][col]; }
        stats[(size_t)b * S2M2_EVAL_WORDS + w] = lo + (hi << 32);
    }
}

static int eval_impl(const s2m2_eval_desc* d, void* stream) {
    S2M2_REQUIRE(d != nullptr, "disp_eval: null descriptor");
    if (int rc = refuse_while_recording("disp_eval")) return rc;
    S2M2_REQUIRE(d->disp && d->gt && d->stats && d->workspace, "disp_eval: null pointer (disp / gt / stats / workspace)");
    S2M2_REQUIRE((d->occ == nullptr) == (d->conf == nullptr), "disp_eval: occ and conf come together (exactly one of them is a null pointer)");
    if (int rc = check_padded_maps("disp_eval", "ground truth", d->B, d->H, d->W, d->Hp, d->Wp)) return rc;
    S2M2_REQUIRE(d->nthr >= 0 && d->nthr <= S2M2_EVAL_MAX_THR, "disp_eval: nthr=%d is outside 0..%d", d->nthr, S2M2_EVAL_MAX_THR);
    for (int t = 0; t < d->nthr; ++t)
        S2M2_REQUIRE(isfinite(d->thr[t]) && d->thr[t] > (t ? d->thr[t - 1] : 0.f),
                     "disp_eval: thresholds must be finite, > 0 and strictly increasing (thr[%d]=%g)", t, (double)d->thr[t]);
    S2M2_REQUIRE(isfinite(d->d1_abs) && isfinite(d->d1_rel), "disp_eval: d1_abs and d1_rel must be finite (%g, %g)", (double)d->d1_abs,
                 (double)d->d1_rel);
    S2M2_REQUIRE(isfinite(d->conf_min) && isfinite(d->occ_min), "disp_eval: conf_min and occ_min must be finite (%g, %g)", (double)d->conf_min,
                 (double)d->occ_min);
    S2M2_REQUIRE(!isnan(d->gt_min), "disp_eval: gt_min is NaN (-inf means: every finite gt is valid)");
    S2M2_REQUIRE((((uintptr_t)d->disp | (uintptr_t)d->occ | (uintptr_t)d->conf | (uintptr_t)d->gt) & 3) == 0,
                 "disp_eval: fp32 tensors must be 4-byte aligned");
    S2M2_REQUIRE((((uintptr_t)d->workspace | (uintptr_t)d->stats) & 7) == 0, "disp_eval: workspace and stats must be 8-byte aligned");

    EvalParams p;
    p.disp = d->disp; p.occ = d->occ; p.conf = d->conf; p.gt = d->gt; p.region = d->region;
    p.part = static_cast<unsigned*>(d->workspace);
    p.H = d->H; p.W = d->W; p.Hp = d->Hp; p.Wp = d->Wp;
    p.oy = (d->Hp - d->H) / 2; p.ox = (d->Wp - d->W) / 2;
    p.rows_per_tile = eval_tile_rows(d->H, d->W);
    p.tiles = tiles(d->H, p.rows_per_tile);
    p.nthr = d->nthr;
    p.gt_vec = ((uintptr_t)d->gt & 15) == 0;
    p.region_vec = ((uintptr_t)d->region & 3) == 0;
    for (int t = 0; t < S2M2_EVAL_MAX_THR; ++t) p.thr[t] = t < d->nthr ? d->thr[t] : INFINITY;
    p.d1_abs = d->d1_abs; p.d1_rel = d->d1_rel; p.gt_min = d->gt_min; p.conf_min = d->conf_min; p.occ_min = d->occ_min;
    const bool vec = d->Wp % 4 == 0 && (((uintptr_t)d->disp | (uintptr_t)d->occ | (uintptr_t)d->conf) & 15) == 0;
    const bool conf = d->conf != nullptr;
    const dim3 grid(p.tiles, d->B), block(kRasterThreads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    if (vec) rc = conf ? launch<eval_tile_kernel<true, true>>("disp_eval (tiles)", grid, block, 0, s, p)
                       : launch<eval_tile_kernel<true, false>>("disp_eval (tiles)", grid, block, 0, s, p);
    else rc = conf ? launch<eval_tile_kernel<false, true>>("disp_eval (tiles)", grid, block, 0, s, p)
                   : launch<eval_tile_kernel<false, false>>("disp_eval (tiles)", grid, block, 0, s, p);
    if (rc) return rc;
    const dim3 sum_grid((S2M2_EVAL_WORDS + kEvalSumWords - 1) / kEvalSumWords, d->B);
    return launch<eval_sum_kernel>("disp_eval (sum)", sum_grid, dim3(kEvalSumThreads), 0, s, static_cast<const unsigned*>(p.part), d->stats, p.tiles);
}

}  // namespace s2m2

extern "C" int s2m2_eval_tile_rows(int H, int W) { return s2m2::raster_extents_ok(1, H, W) ? s2m2::eval_tile_rows(H, W) : 0; }

extern "C" size_t s2m2_eval_workspace_bytes(int B, int H, int W) {
    using namespace s2m2;
    if (!raster_extents_ok(B, H, W)) return 0;
    return round256((size_t)B * tiles(H, eval_tile_rows(H, W)) * kEvalPart * sizeof(unsigned));
}

extern "C" int s2m2_disp_eval(const s2m2_eval_desc* desc, void* stream) { return s2m2::eval_impl(desc, stream); }
