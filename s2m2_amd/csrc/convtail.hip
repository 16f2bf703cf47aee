// K19 -- the second half of a ConvBlock2D in ONE launch, for the grids K14 does not take (s2m2_conv_block_tail).
//
// Reference: ConvBlock2D.forward (attentions.py:255-281):   out = convs.2(GELU(convs.0(z))) + convs_1x.2(ReLU(convs_1x.0(z)))
// Above K14's grids the block is three launches: the K9 chain on the 1x1 branch (reads z, writes b), K5 v5 on convs.0 (t = GELU(...)) and K5 v5
// on convs.2 with the residual epilogue (reads t and b).  The 1x1 branch needs no halo: the block that adds it can compute it on its own
// patch, from the patch's own pixels of z, in front of the K loop of convs.2 -- no recompute, one launch less, and b never exists in memory.
//
//   block = v5's: a 2x32, 4x32 or 4x40 patch of output pixels (convtail_select.h) x ALL C output channels, one wave per 32 couts;
//   pre-phase:  the patch's pixels of z -> LDS (no halo); convs_1x.0 from K9's fragment stream in K9's channel order, bias + ReLU rounded to
//               fp16 into the ReLU tile (which aliases the z tile); convs_1x.2 from the ReLU tile; s1 = fp16(acc + bb) stays in registers, packed;
//   main phase: v5's K loop on t: the halo tile of one 128-channel chunk in LDS, the weights through the 8-deep untracked ring (frag_ring.h),
//               order (chunk, tap, k16 step).  The ring starts only after the pre-phase's tracked loads are consumed;
//   epilogue:   fp16(fp16(acc + b2) + s1) in registers -> staged through LDS -> coalesced 16-byte stores.
// Rounding points and summation orders are K9's output store and K5's EPI_ADD: bit-identical to the two launches (tests/test_hip_convtail.py).
// fp16, C = 128 / 256.
#include "common.h"
#include "launch.h"
#include "plan.h"
#include "epilogue.h"
#include "frag_ring.h"
#include "convtail_select.h"
#include <stdint.h>

namespace s2m2 {

struct CtArgs {
    const half_t* t; const half_t* z; half_t* out;
    unsigned ts, zs, os;                        // elements between pixels (a tensor spans less than 2^31 elements: 32-bit offsets)
    int N, H, W, tiles_x, tiles_y;
    const raw16_t* w2;                          // convs.2: K5 v5 fragment stream
    const raw16_t* wa; const raw16_t* wb;       // convs_1x.0 / convs_1x.2: K9 fragment order
    const float* b2; const float* ba; const float* bb;   // biases (or null)
    const void* zero;
};

template <int C_, int PH_, int PW_>
struct CtCfg {
    static constexpr int C = C_, PH = PH_, PW = PW_, NW = C_ / 32, NT = 64 * NW, KS = 8, CH = 128, NCHUNK = C_ / 128;
    static constexpr int NP = PH * PW, MT = NP / 32;                                         // output patch, MFMA pixel tiles (raster order)
    static constexpr int HH = PH + 2, HW = PW + 2, NHALO = HH * HW;                          // halo tile of t
    using Halo = HaloGeom<NT, CH, NHALO>;                                                    // one 128-channel chunk of it and its loader (frag_ring.h)
    static constexpr int RS = Halo::RS, TRS = C + 8, PPX = Halo::PPX, RPI = Halo::RPI, A_IT = Halo::A_IT, AROWS = Halo::AROWS;
    static constexpr size_t A_BYTES = Halo::A_BYTES;
    static constexpr size_t Z_BYTES = (size_t)NP * TRS * 2;                                  // z tile = ReLU tile = staging tile: [NP][TRS]
    static constexpr size_t OFF_B = ((A_BYTES > Z_BYTES ? A_BYTES : Z_BYTES) + 15) / 16 * 16, LDS_BYTES = OFF_B + 3 * C * 4;
    static constexpr int ZP = C / 8, SP = NP * ZP / NT;                                      // 16-byte pieces per pixel / per thread (z tile, store)
    static_assert(NP % 32 == 0 && NP * ZP % NT == 0 && LDS_BYTES <= 160 * 1024, "conv block tail tile");
    static_assert(C != 128 || LDS_BYTES <= 80 * 1024, "C = 128: two blocks per CU");
};

template <typename CFG>
__global__ __launch_bounds__(CFG::NT, 2) void conv_tail_kernel(CtArgs p) {
    constexpr int C = CFG::C, PW = CFG::PW, KS = CFG::KS, RS = CFG::RS, TRS = CFG::TRS, HW = CFG::HW, MT = CFG::MT, NCHUNK = CFG::NCHUNK;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* Zt = reinterpret_cast<half_t*>(smem);                // z tile [NP][TRS]; then the ReLU tile; after the K loop the staging tile
    half_t* Ah = reinterpret_cast<half_t*>(smem);                // halo tile of t [AROWS][RS] (main phase)
    float* bvec = reinterpret_cast<float*>(smem + CFG::OFF_B);   // b2 | ba | bb
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);     // cout tile of this wave
    int bx = blockIdx.x;                                         // patch <-> block id as in v5: convs.0 left this patch of t in this XCD's L2
    const int tx = bx % p.tiles_x; bx /= p.tiles_x;
    const int ty = bx % p.tiles_y;
    const int n = bx / p.tiles_y;
    const int y0 = ty * CFG::PH, x0 = tx * PW;
    const half_t* zp = static_cast<const half_t*>(p.zero);

    for (int i = tid; i < 3 * C; i += CFG::NT) {
        const int k = i / C, c = i - k * C;
        const float* src = k == 0 ? p.b2 : k == 1 ? p.ba : p.bb;
        bvec[i] = src ? src[c] : 0.f;
    }
    // ---- this thread's 16-byte pieces of the patch: piece pcc of patch pixel r (raster order), for the z tile now and for the store at the end
    // (recomputed there from a thread id the compiler cannot match with this one: ten pixel indices held through the K loop are registers the
    // 4x40 form does not have)
    auto piece_pix = [&](int t, int it) __attribute__((always_inline)) -> int {
        const int r = (t + CFG::NT * it) / CFG::ZP;
        const int py = r / PW, yy = y0 + py, xx = x0 + (r - py * PW);
        return (yy < p.H && xx < p.W) ? (n * p.H + yy) * p.W + xx : -1;
    };
    {
        raw16_t rz[CFG::SP];
#pragma unroll
        for (int it = 0; it < CFG::SP; ++it) {
            const int s = tid + CFG::NT * it, r = s / CFG::ZP, pcc = s - r * CFG::ZP;
            const int m = piece_pix(tid, it);
            rz[it] = global_load16(m >= 0 ? p.z + ((unsigned)m * p.zs + pcc * 8) : zp);
        }
#pragma unroll
        for (int it = 0; it < CFG::SP; ++it) {
            const int s = tid + CFG::NT * it, r = s / CFG::ZP, pcc = s - r * CFG::ZP;
            *reinterpret_cast<raw16_t*>(Zt + (size_t)r * TRS + pcc * 8) = rz[it];
        }
    }
    __syncthreads();

    // ---- pre-phase: s1 = fp16(convs_1x.2(fp16(ReLU(convs_1x.0(z) + ba))) + bb) on the patch, packed as the lane holds it
    // (pinned as packed pairs: left to itself the compiler keeps the 16 halves of a tile in 16 registers through the K loop)
    unsigned s1[MT][8];
    {
        float16_t accA[MT];
        tile_1x1<MT, KS, C, TRS>(accA, Zt, p.wa + (size_t)wv * (C / 16) * 64 + lane, l31, hi);
        __syncthreads();                                         // every wave is done with the z tile (the ReLU tile aliases it)
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            half_t* rrow = Zt + (size_t)(32 * i + l31) * TRS + wv * 32 + 4 * hi;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const float4_t bv = *reinterpret_cast<const float4_t*>(bvec + C + wv * 32 + 8 * gq + 4 * hi);
                half4_t h;
#pragma unroll
                for (int e = 0; e < 4; ++e) h[e] = from_f32<half_t>(fmaxf(accA[i][4 * gq + e] + bv[e], 0.f) * 1.0f);
                *reinterpret_cast<half4_t*>(rrow + 8 * gq) = h;
            }
        }
        __syncthreads();
        float16_t accB[MT];
        tile_1x1<MT, KS, C, TRS>(accB, Zt, p.wb + (size_t)wv * (C / 16) * 64 + lane, l31, hi);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const float4_t bv = *reinterpret_cast<const float4_t*>(bvec + 2 * C + wv * 32 + 8 * gq + 4 * hi);
#pragma unroll
                for (int e = 0; e < 4; e += 2) {
                    const half2_t pr = {from_f32<half_t>((accB[i][4 * gq + e] + bv[e]) * 1.0f), from_f32<half_t>((accB[i][4 * gq + e + 1] + bv[e + 1]) * 1.0f)};
                    unsigned u = __builtin_bit_cast(unsigned, pr);
                    asm volatile("" : "+v"(u));
                    s1[i][2 * gq + e / 2] = u;
                }
            }
    }
    __syncthreads();                                             // every wave is done with the ReLU tile (the halo tile aliases it)

    // ---- main phase: convs.2 on t, v5's loop.  Halo loader: piece pc of halo pixels prow + RPI * it.  Its addresses come from a thread id the
    // compiler cannot match with `tid`: hoisted out of the chunk loop (or above the pre-phase) they are 2 * A_IT registers the 4x40 form lacks
    auto load_halo = [&](int chunk) __attribute__((always_inline)) {
        int t = tid;
        asm volatile("" : "+v"(t));
        const int pc = t % CFG::PPX, prow = t / CFG::PPX;
        raw16_t ra[CFG::A_IT];
#pragma unroll
        for (int it = 0; it < CFG::A_IT; ++it) {
            const int hp = prow + CFG::RPI * it;
            const int hy = hp / HW, hx = hp - hy * HW;
            const int yy = y0 - 1 + hy, xx = x0 - 1 + hx;
            const bool ok = hp < CFG::NHALO && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
            const half_t* src = ok ? p.t + ((unsigned)((n * p.H + yy) * p.W + xx) * p.ts + chunk * CFG::CH + pc * 8) : zp;
            ra[it] = global_load16(src);
        }
        // every request is consumed, unconditionally (rows past the halo are padding): conv.hip, load_halo
#pragma unroll
        for (int it = 0; it < CFG::A_IT; ++it) *reinterpret_cast<raw16_t*>(Ah + (size_t)(prow + CFG::RPI * it) * RS + pc * 8) = ra[it];
    };
    const int nfrag = NCHUNK * 9 * KS;
    const raw16_t* wf = p.w2 + (size_t)wv * nfrag * 64 + lane;
    raw16_t ring[KS];
    // frag_ring.h: ring_start, kept inline (the call moves this kernel's code object).  The halo tile's tracked loads are younger, so the
    // compiler's waits at the stash cover the ring as well (conv.hip)
#pragma unroll
    for (int s = 0; s < KS - 1; ++s) global_load16_async(ring[s], wf + (size_t)s * 64);
    load_halo(0);
    __syncthreads();
    float16_t acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    int poff[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int q = 32 * i + l31, qy = q / PW;
        poff[i] = (qy * HW + (q - qy * PW)) * RS + hi * 8;
    }
    int g = 0;
#pragma unroll 1
    for (int chunk = 0; chunk < NCHUNK; ++chunk) {
        if (chunk > 0) {
            wait_vmcnt<0>();                                     // the ring's requests land before tracked loads are mixed in
            __syncthreads();                                     // every wave is done with the previous chunk's tile
            load_halo(chunk);
            __syncthreads();
        }
        int ky = 0, kx = 0;
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            cb_steps<MT, KS>(acc, Ah + (ky * HW + kx) * RS, poff, ring, wf, g, nfrag);
            if (++kx == 3) { kx = 0; ++ky; }
        }
    }
    ring_drain(ring);
    __syncthreads();                                             // the staging tile aliases the halo tile

    // ---- epilogue: out = fp16(fp16(convs.2 + b2) + s1): K5's EPI_ADD on K9's output, staged for coalesced 16-byte stores
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        half_t* srow = Zt + (size_t)(32 * i + l31) * TRS + wv * 32 + 4 * hi;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const float4_t b2 = *reinterpret_cast<const float4_t*>(bvec + wv * 32 + 8 * gq + 4 * hi);
            half4_t h;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const half_t m = from_f32<half_t>((acc[i][4 * gq + e] + b2[e]) * 1.0f);
                h[e] = from_f32<half_t>((float)m + (float)__builtin_bit_cast(half2_t, s1[i][2 * gq + e / 2])[e & 1]);
            }
            *reinterpret_cast<half4_t*>(srow + 8 * gq) = h;
        }
    }
    __syncthreads();
    int tid_s = tid;
    asm volatile("" : "+v"(tid_s));
#pragma unroll
    for (int it = 0; it < CFG::SP; ++it) {
        const int s = tid_s + CFG::NT * it, r = s / CFG::ZP, pcc = s - r * CFG::ZP;
        const int m = piece_pix(tid_s, it);
        if (m < 0) continue;
        *reinterpret_cast<raw16_t*>(p.out + ((unsigned)m * p.os + pcc * 8)) = *reinterpret_cast<const raw16_t*>(Zt + (size_t)r * TRS + pcc * 8);
    }
}

template <int C, int PH, int PW>
static int launch_ct(const CtArgs& a0, hipStream_t st) {
    using CFG = CtCfg<C, PH, PW>;
    CtArgs a = a0;
    a.tiles_x = (a.W + PW - 1) / PW;
    a.tiles_y = (a.H + PH - 1) / PH;
    return launch<conv_tail_kernel<CFG>>("conv_block_tail", dim3((unsigned)(a.N * a.tiles_x * a.tiles_y)), dim3(CFG::NT), CFG::LDS_BYTES, st, a);
}

template <int C>
static int launch_ct_patch(const CtArgs& a, hipStream_t st, ConvTailPatch pt) {
    if (pt.pw == 40) return launch_ct<C, 4, 40>(a, st);
    return pt.ph == 4 ? launch_ct<C, 4, 32>(a, st) : launch_ct<C, 2, 32>(a, st);
}

}  // namespace s2m2

extern "C" int s2m2_conv_block_tail_supported(int C, int H, int W, int dtype) {
    return dtype == S2M2_F16 && (C == 128 || C == 256) && H >= 1 && W >= 1;
}

static int conv_block_tail_impl(const s2m2_convtail_desc* d, void* stream) {
    using namespace s2m2;
    S2M2_REQUIRE(d, "conv_block_tail: null descriptor");
    S2M2_REQUIRE(d->dtype == S2M2_F16, "conv_block_tail: dtype=%d (fp16 only)", d->dtype);
    S2M2_REQUIRE(d->C == 128 || d->C == 256, "conv_block_tail: C=%d (128 or 256)", d->C);
    S2M2_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && (long long)d->N * d->H * d->W < (1LL << 24), "conv_block_tail: bad shape");
    const long long pixels = (long long)d->N * d->H * d->W;
    constexpr const char* E = "conv_block_tail";
    if (check_activation(E, "t", d->t, d->t_stride, pixels, d->C, 16, true) || check_activation(E, "z", d->z, d->z_stride, pixels, d->C, 16, true) ||
        check_activation(E, "out", d->out, d->out_stride, pixels, d->C, 16, true)) return 1;
    if (check_weight_stream(E, "w_conv2", d->w_conv2) || check_weight_stream(E, "w_1x0", d->w_1x0) || check_weight_stream(E, "w_1x2", d->w_1x2)) return 1;
    if (check_disjoint(E, "t", d->t, d->t_stride, d->out, d->out_stride, pixels, d->C) ||
        check_disjoint(E, "z", d->z, d->z_stride, d->out, d->out_stride, pixels, d->C)) return 1;
    const bool forced = d->patch_rows != 0 || d->patch_cols != 0;
    const ConvTailPatch pt = conv_tail_patch(d->N, d->H, d->W, d->C, d->patch_rows, d->patch_cols);
    S2M2_REQUIRE(!forced || (pt.ph == d->patch_rows && pt.pw == d->patch_cols), "conv_block_tail: patch %d x %d (2 x 32, 4 x 32 or 4 x 40)",
                 d->patch_rows, d->patch_cols);
    CtArgs a;
    a.t = static_cast<const half_t*>(d->t); a.z = static_cast<const half_t*>(d->z); a.out = static_cast<half_t*>(d->out);
    a.ts = (unsigned)d->t_stride; a.zs = (unsigned)d->z_stride; a.os = (unsigned)d->out_stride;
    a.N = d->N; a.H = d->H; a.W = d->W;
    a.w2 = static_cast<const raw16_t*>(d->w_conv2); a.wa = static_cast<const raw16_t*>(d->w_1x0); a.wb = static_cast<const raw16_t*>(d->w_1x2);
    a.b2 = d->b_conv2; a.ba = d->b_1x0; a.bb = d->b_1x2;
    if (bind_zero_page(a, "conv_block_tail")) return 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return d->C == 256 ? launch_ct_patch<256>(a, st, pt) : launch_ct_patch<128>(a, st, pt);
}
// the name a recording stores for this call and the name the loader's table maps back (plan.h): one constant, so the two cannot drift apart
static constexpr char kConvTailEntry[] = "s2m2_conv_block_tail";
extern "C" int s2m2_conv_block_tail(const s2m2_convtail_desc* d, void* stream) {
    return s2m2::plan_dispatch_desc<s2m2_convtail_desc>(kConvTailEntry, &conv_block_tail_impl, d, stream);
}
S2M2_PLAN_DESC_ENTRY(kConvTailEntry, conv_block_tail_impl)
