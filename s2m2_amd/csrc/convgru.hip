// K17 -- one ConvGRU half (refinenet.py:7-36) in ONE launch (s2m2_conv_gru):
//
//   z  = sigmoid(convz([h, x]))      r = sigmoid(convr([h, x]))      q = tanh(convq([r * h, x]))      h' = (1 - z) * h + z * q
//
// with 1x3 or 3x1 taps, fp16, hidden and input width 128.  The two launches this replaces (K5 v5 on the stacked z | r layer with the r * h
// epilogue, then the candidate layer with the blend epilogue) each load a 69 KB halo tile per 128-channel chunk for three taps of MFMA work,
// and z and r * h make an HBM round trip between them.  The candidate layer needs r * h on the output patch plus ONE pixel along the tap
// axis only, so here
//
//   block = a patch of 160 output pixels (4 x 40 for 1x3 taps, 8 x 20 for 3x1) x all 128 channels, 8 waves;
//   tiles:   h and x on the patch plus two pixels along the tap axis on each side, both in LDS behind one load phase;
//   phase 1: waves 0-3 compute z (32 couts each) on the patch, waves 4-7 compute r on the patch plus its one-pixel ring (recomputed by the
//            neighbouring blocks: 1.2 - 1.4 x the MFMAs of the unfused r layer); r * h overwrites the h tile in LDS.  Ring pixels
//            outside the image hold h = 0, so r * h = 0 there: the candidate layer's zero padding;
//   phase 2: waves 0-3 run the candidate layer from the LDS-resident r * h and x tiles; z and tanh(...) are staged over the dead tiles and
//            every thread blends 16-byte pieces with h from global memory -> coalesced store.
//   weights: the fragment streams of K5 v5 as they are (the stacked z | r stream, the candidate layer's stream), through the 8-deep
//            untracked ring with counted waits of conv_frag_kernel (frag_ring.h).
// Accumulation order = K5 v5's (chunk h / r * h, chunk x) x tap x k16 step, and z, r * h, tanh(...) and the blend are rounded where the two
// launches round them: bit-identical to them (tests/test_hip_conv_gru.py).
#include "common.h"
#include "launch.h"
#include "plan.h"
#include "epilogue.h"
#include "frag_ring.h"
#include <stdint.h>

namespace s2m2 {

struct GruArgs {
    const half_t* h; const half_t* x; half_t* out;
    long long hs, xs, os;                       // elements between pixels
    int N, H, W, tiles_x, tiles_y;
    const raw16_t* wzr; const raw16_t* wq;      // K5 v5 fragment streams: z | r stacked (8 cout tiles), candidate layer (4 cout tiles)
    const float* bzr; const float* bq;          // biases (or null)
    const void* zero;
};

// VERT: 3x1 taps (the tap axis is y), else 1x3 (x)
template <bool VERT_>
struct GruCfg {
    static constexpr bool VERT = VERT_;
    static constexpr int C = 128, KS = 8, NWAVES = 8, NT = 64 * NWAVES, NTAP = 3, NFRAG = 2 * NTAP * KS;
    static constexpr int PH = VERT ? 8 : 4, PW = VERT ? 20 : 40, NP = PH * PW, MTZ = NP / 32;           // output patch
    static constexpr int RH = VERT ? PH + 2 : PH, RW = VERT ? PW : PW + 2, NR = RH * RW, MTR = (NR + 31) / 32;   // patch + ring (r * h)
    static constexpr int TH = VERT ? PH + 4 : PH, TW = VERT ? PW : PW + 4, NTILE = TH * TW;             // input tiles
    static constexpr int TAPS = VERT ? TW : 1;                                                          // tile pixels between two taps
    using Halo = HaloGeom<NT, C, NTILE>;                                                                // one input tile and its loader (frag_ring.h)
    static constexpr int RS = Halo::RS, CRS = C + 8, PPX = Halo::PPX, RPI = Halo::RPI, A_IT = Halo::A_IT, AROWS = Halo::AROWS;
    static constexpr size_t A_BYTES = Halo::A_BYTES;
    static constexpr size_t STAGE_BYTES = (size_t)NP * CRS * 2;                                         // z / tanh staging (alias the tiles)
    static constexpr size_t OFF_X = A_BYTES, OFF_B = 2 * A_BYTES, LDS_BYTES = OFF_B + 3 * C * 4;
    static constexpr int PCR = C / 8, SP = NP * PCR / NT;                                               // staged pieces per thread
    static_assert(NP % 32 == 0 && NP * PCR % NT == 0 && STAGE_BYTES <= A_BYTES && LDS_BYTES <= 160 * 1024, "conv gru tile");
};

// one layer's K loop on MT pixel tiles: (tile t0, tile t1) x tap x k16 step against this wave's fragment stream, v5's order
template <typename CFG, int MT>
__device__ __forceinline__ void gru_layer(float16_t (&acc)[MT], const half_t* t0, const half_t* t1, const int (&poff)[MT], const raw16_t* wf) {
    constexpr int KS = CFG::KS;
    raw16_t ring[KS];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    ring_start(ring, wf);
    int g = 0;
#pragma unroll 1
    for (int chunk = 0; chunk < 2; ++chunk) {
        const half_t* t = chunk ? t1 : t0;
#pragma unroll 1
        for (int tap = 0; tap < CFG::NTAP; ++tap) cb_steps<MT, KS>(acc, t + tap * CFG::TAPS * CFG::RS, poff, ring, wf, g, CFG::NFRAG);
    }
    ring_drain(ring);
}

// fp16(ACT(acc + bias)) of one accumulator tile, packed as the lane holds it (quad gq: couts 8 gq + 4 hi .. + 3 of the wave's 32).  The empty
// asm pins the fp32 value: the conversion must round the activation's result like K5's staging pass does, not fuse with its last fma.
template <int ACT>
__device__ __forceinline__ void gate16(half4_t (&o)[4], const float16_t& acc, const float* bv, int hi) {
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        const float4_t b = *reinterpret_cast<const float4_t*>(bv + 8 * gq + 4 * hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = activate<ACT>(acc[4 * gq + e] + b[e]);
            asm volatile("" : "+v"(v));
            o[gq][e] = from_f32<half_t>(v);
        }
    }
}

template <typename CFG>
__global__ __launch_bounds__(CFG::NT) void conv_gru_kernel(GruArgs p) {
    constexpr int RS = CFG::RS, CRS = CFG::CRS, TW = CFG::TW, PW = CFG::PW, RW = CFG::RW, MTZ = CFG::MTZ, MTR = CFG::MTR, C = CFG::C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* Ht = reinterpret_cast<half_t*>(smem);                // h tile [AROWS][RS], r * h on the ring after phase 1; later the z staging tile
    half_t* Xt = reinterpret_cast<half_t*>(smem + CFG::OFF_X);   // x tile; later the tanh staging tile
    half_t* Zs = Ht;
    half_t* Qs = Xt;
    float* bvec = reinterpret_cast<float*>(smem + CFG::OFF_B);   // bz | br | bq
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);     // cout tile of the stacked z | r layer: 0-3 z, 4-7 r
    int bx = blockIdx.x;
    const int tx = bx % p.tiles_x; bx /= p.tiles_x;
    const int ty = bx % p.tiles_y;
    const int n = bx / p.tiles_y;
    const int y0 = ty * CFG::PH, x0 = tx * PW;
    const half_t* zp = static_cast<const half_t*>(p.zero);

    for (int i = tid; i < 3 * C; i += CFG::NT) {
        const float* src = i < 2 * C ? p.bzr : p.bq;
        bvec[i] = src ? src[i < 2 * C ? i : i - 2 * C] : 0.f;
    }
    // ---- both input tiles: piece pc of tile pixels prow + RPI * it (pixels outside the image and rows past the tile read the zero page)
    {
        const int pc = tid % CFG::PPX, prow = tid / CFG::PPX;
        long long apix[CFG::A_IT];
#pragma unroll
        for (int it = 0; it < CFG::A_IT; ++it) {
            const int tp = prow + CFG::RPI * it;
            const int tyy = tp / TW, txx = tp - tyy * TW;
            const int yy = y0 + tyy - (CFG::VERT ? 2 : 0), xx = x0 + txx - (CFG::VERT ? 0 : 2);
            const bool ok = tp < CFG::NTILE && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
            apix[it] = ok ? ((long long)(n * p.H + yy) * p.W + xx) : -1;
        }
        raw16_t ra[CFG::A_IT];
#pragma unroll
        for (int it = 0; it < CFG::A_IT; ++it) ra[it] = global_load16(apix[it] >= 0 ? p.h + apix[it] * p.hs + pc * 8 : zp);
#pragma unroll
        for (int it = 0; it < CFG::A_IT; ++it) *reinterpret_cast<raw16_t*>(Ht + (size_t)(prow + CFG::RPI * it) * RS + pc * 8) = ra[it];
#pragma unroll
        for (int it = 0; it < CFG::A_IT; ++it) ra[it] = global_load16(apix[it] >= 0 ? p.x + apix[it] * p.xs + pc * 8 : zp);
#pragma unroll
        for (int it = 0; it < CFG::A_IT; ++it) *reinterpret_cast<raw16_t*>(Xt + (size_t)(prow + CFG::RPI * it) * RS + pc * 8) = ra[it];
    }
    __syncthreads();

    // tile offsets (elements) of this lane's pixel at tap 0.  Patch pixel q = 32 i + l31 in raster order sits at tile (py, px + 2) / (py + 2, px):
    // tap 0 reads one pixel before it along the tap axis; ring pixel q sits one pixel before the patch, tap 0 reads the tile's first pixel.
    int poffZ[MTZ], poffR[MTR];
#pragma unroll
    for (int i = 0; i < MTZ; ++i) {
        const int q = 32 * i + l31, py = q / PW, px = q - py * PW;
        poffZ[i] = ((CFG::VERT ? (py + 1) * TW + px : py * TW + px + 1)) * RS + hi * 8;
    }
#pragma unroll
    for (int i = 0; i < MTR; ++i) {
        int q = 32 * i + l31;
        q = q < CFG::NR ? q : CFG::NR - 1;                        // lanes past the ring recompute its last pixel (never written)
        const int ry = q / RW, rx = q - ry * RW;
        poffR[i] = (ry * TW + rx) * RS + hi * 8;
    }

    // ---- phase 1: the stacked z | r layer.  gate[i]: fp16 z of patch tile i (waves 0-3) / fp16 r of ring tile i (waves 4-7)
    const raw16_t* wf1 = p.wzr + (size_t)wv * CFG::NFRAG * 64 + lane;
    half4_t gate[MTR][4];
    if (wv < 4) {
        float16_t acc[MTZ];
        gru_layer<CFG, MTZ>(acc, Ht, Xt, poffZ, wf1);
#pragma unroll
        for (int i = 0; i < MTZ; ++i) gate16<S2M2_ACT_SIGMOID>(gate[i], acc[i], bvec + wv * 32, hi);
    } else {
        float16_t acc[MTR];
        gru_layer<CFG, MTR>(acc, Ht, Xt, poffR, wf1);
#pragma unroll
        for (int i = 0; i < MTR; ++i) gate16<S2M2_ACT_SIGMOID>(gate[i], acc[i], bvec + wv * 32, hi);
    }
    __syncthreads();                                             // every wave is done reading h
    if (wv >= 4) {
        // r * h in place over the ring's h (K5: EPI_MUL on the staged fp16 r)
#pragma unroll
        for (int i = 0; i < MTR; ++i) {
            if (32 * i + l31 < CFG::NR) {
                half_t* row = Ht + (poffR[i] - hi * 8) + CFG::TAPS * RS + (wv - 4) * 32 + 4 * hi;
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    half4_t hv = *reinterpret_cast<const half4_t*>(row + 8 * gq);
#pragma unroll
                    for (int e = 0; e < 4; ++e) hv[e] = from_f32<half_t>(to_f32(gate[i][gq][e]) * to_f32(hv[e]));
                    *reinterpret_cast<half4_t*>(row + 8 * gq) = hv;
                }
            }
        }
    }
    __syncthreads();

    // ---- phase 2: the candidate layer on the patch from the r * h and x tiles (waves 0-3, 32 couts each)
    half4_t cand[MTZ][4];
    if (wv < 4) {
        float16_t acc[MTZ];
        gru_layer<CFG, MTZ>(acc, Ht, Xt, poffZ, p.wq + (size_t)wv * CFG::NFRAG * 64 + lane);
#pragma unroll
        for (int i = 0; i < MTZ; ++i) gate16<S2M2_ACT_TANH>(cand[i], acc[i], bvec + 2 * C + wv * 32, hi);
    }
    __syncthreads();                                             // the staging tiles alias the input tiles

    // ---- blend and store: h for this thread's pieces is requested now and arrives under the staging pass
    raw16_t hreg[CFG::SP];
    long long opix[CFG::SP];
#pragma unroll
    for (int it = 0; it < CFG::SP; ++it) {
        const int s = tid + CFG::NT * it, r = s / CFG::PCR, pcc = s - r * CFG::PCR;
        const int py = r / PW, yy = y0 + py, xx = x0 + (r - py * PW);
        opix[it] = (yy < p.H && xx < p.W) ? ((long long)(n * p.H + yy) * p.W + xx) : -1;
        hreg[it] = global_load16(opix[it] >= 0 ? p.h + opix[it] * p.hs + pcc * 8 : zp);
    }
    if (wv < 4) {
#pragma unroll
        for (int i = 0; i < MTZ; ++i) {
            const size_t o = (size_t)(32 * i + l31) * CRS + wv * 32 + 4 * hi;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                *reinterpret_cast<half4_t*>(Zs + o + 8 * gq) = gate[i][gq];
                *reinterpret_cast<half4_t*>(Qs + o + 8 * gq) = cand[i][gq];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < CFG::SP; ++it) {
        const int s = tid + CFG::NT * it, r = s / CFG::PCR, pcc = s - r * CFG::PCR;
        if (opix[it] < 0) continue;
        Vec16<half_t> v = *reinterpret_cast<const Vec16<half_t>*>(Qs + (size_t)r * CRS + pcc * 8);
        const Vec16<half_t> zv = *reinterpret_cast<const Vec16<half_t>*>(Zs + (size_t)r * CRS + pcc * 8);
        aux_combine(v, (int)S2M2_EPI_GRU, zv, __builtin_bit_cast(Vec16<half_t>, hreg[it]));     // K5's blend, one rounding
        *reinterpret_cast<Vec16<half_t>*>(p.out + opix[it] * p.os + pcc * 8) = v;
    }
}

template <bool VERT>
static int launch_gru(const GruArgs& a0, hipStream_t st) {
    using CFG = GruCfg<VERT>;
    GruArgs a = a0;
    a.tiles_x = (a.W + CFG::PW - 1) / CFG::PW;
    a.tiles_y = (a.H + CFG::PH - 1) / CFG::PH;
    return launch<conv_gru_kernel<CFG>>("conv_gru", dim3((unsigned)(a.N * a.tiles_x * a.tiles_y)), dim3(CFG::NT), CFG::LDS_BYTES, st, a);
}

}  // namespace s2m2

extern "C" int s2m2_conv_gru_supported(int C, int H, int W, int dtype) {
    return dtype == S2M2_F16 && C == 128 && H >= 1 && W >= 1;
}

static int conv_gru_impl(const s2m2_convgru_desc* d, void* stream) {
    using namespace s2m2;
    S2M2_REQUIRE(d, "conv_gru: null descriptor");
    S2M2_REQUIRE(d->dtype == S2M2_F16 && d->C == 128, "conv_gru: C=%d dtype=%d (fp16, C = 128)", d->C, d->dtype);
    S2M2_REQUIRE((d->KH == 3 && d->KW == 1) || (d->KH == 1 && d->KW == 3), "conv_gru: %d x %d taps (3 x 1 or 1 x 3)", d->KH, d->KW);
    S2M2_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && (long long)d->N * d->H * d->W < (1LL << 24), "conv_gru: bad shape");
    const long long pixels = (long long)d->N * d->H * d->W;
    constexpr const char* E = "conv_gru";
    if (check_activation(E, "h", d->h, d->h_stride, pixels, d->C) || check_activation(E, "x", d->x, d->x_stride, pixels, d->C) ||
        check_activation(E, "out", d->out, d->out_stride, pixels, d->C)) return 1;
    if (check_weight_stream(E, "w_zr", d->w_zr) || check_weight_stream(E, "w_q", d->w_q)) return 1;
    if (check_disjoint(E, "h", d->h, d->h_stride, d->out, d->out_stride, pixels, d->C) ||
        check_disjoint(E, "x", d->x, d->x_stride, d->out, d->out_stride, pixels, d->C)) return 1;
    GruArgs a;
    a.h = static_cast<const half_t*>(d->h); a.x = static_cast<const half_t*>(d->x); a.out = static_cast<half_t*>(d->out);
    a.hs = d->h_stride; a.xs = d->x_stride; a.os = d->out_stride;
    a.N = d->N; a.H = d->H; a.W = d->W;
    a.wzr = static_cast<const raw16_t*>(d->w_zr); a.wq = static_cast<const raw16_t*>(d->w_q);
    a.bzr = d->b_zr; a.bq = d->b_q;
    if (bind_zero_page(a, "conv_gru")) return 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return d->KH == 3 ? launch_gru<true>(a, st) : launch_gru<false>(a, st);
}
// the name a recording stores for this call and the name the loader's table maps back (plan.h): one constant, so the two cannot drift apart
static constexpr char kConvGruEntry[] = "s2m2_conv_gru";
extern "C" int s2m2_conv_gru(const s2m2_convgru_desc* d, void* stream) {
    return s2m2::plan_dispatch_desc<s2m2_convgru_desc>(kConvGruEntry, &conv_gru_impl, d, stream);
}
S2M2_PLAN_DESC_ENTRY(kConvGruEntry, conv_gru_impl)
