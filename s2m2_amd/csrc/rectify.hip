// K16: the rectifier in front of the forward (include/s2m2_hip.h: s2m2_rectify) -- per output pixel the inverse map of
// cv2.initUndistortRectifyMap through the distortion model, then a bilinear gather with a zero border; one launch for a whole population of
// rectifications (records in device memory) of one raw pair.
// Pixel -> thread map: a lane owns four consecutive output pixels of one row (one 16-byte store per plane), 32 lanes span 128 pixels, the eight
// half-waves of a block take eight consecutive rows: a block is a 128 x 8 output tile, whose source footprint is a compact patch of about the
// same size.  Block order (header: `order`): sample-fastest -- consecutive block ids are the same tile of consecutive records, so the blocks
// that read one source patch are in flight together and the patch is fetched once per L2 -- or tile-fastest.
// The source (3-12 bytes per pixel, shared by every record of a camera) is small against the output (fp32: 12 bytes per pixel and record), so
// the taps are plain global loads that hit L1 / L2, not staged in LDS; measured, the stage is bound by those gathers and the map arithmetic,
// not by its stores.  Loads never leave the source: tap coordinates are clamped into it and the
// contribution of an outside tap is selected away, so there is no divergent branch and no out-of-bounds address for any map value (NaN included).
#include "common.h"
#include "launch.h"
#include "plan.h"

namespace s2m2 {

constexpr int kRectThreads = 256;
constexpr int kRectPx = 4;                                 // consecutive output pixels of a lane
constexpr int kRectTileW = 32 * kRectPx;                   // 128
constexpr int kRectTileH = kRectThreads / 32;              // 8

typedef unsigned char uchar4_t __attribute__((ext_vector_type(4)));

struct RectParams {
    const void* src[2];
    const float* records;
    void* out;
    float* maps;
    int n_src, n_img;
    int Hs, Ws, Hd, Wd;
    int tiles_x, tiles;                                    // tiles of one output image
    int round, tile_fastest;
};

// the three channels of source pixel (y, x), which is inside the source
template <int FMT> __device__ __forceinline__ void rect_fetch(const void* src, int Hs, int Ws, int y, int x, float c[3]) {
    const size_t px = (size_t)y * Ws + x;
    if constexpr (FMT == S2M2_RECTIFY_SRC_U8_HWC) {
        const unsigned char* p = static_cast<const unsigned char*>(src) + px * 3;
        c[0] = (float)p[0]; c[1] = (float)p[1]; c[2] = (float)p[2];
    } else if constexpr (FMT == S2M2_RECTIFY_SRC_U8_CHW) {
        const unsigned char* p = static_cast<const unsigned char*>(src) + px;
        const size_t plane = (size_t)Hs * Ws;
        c[0] = (float)p[0]; c[1] = (float)p[plane]; c[2] = (float)p[2 * plane];
    } else {
        const float* p = static_cast<const float*>(src) + px;
        const size_t plane = (size_t)Hs * Ws;
        c[0] = p[0]; c[1] = p[plane]; c[2] = p[2 * plane];
    }
}

template <int FMT, bool OUT_U8, bool VEC>
__global__ __launch_bounds__(kRectThreads) void rectify_kernel(const RectParams p) {
    int img, tile;
    if (p.tile_fastest) { img = blockIdx.x / p.tiles; tile = blockIdx.x - img * p.tiles; }
    else { tile = blockIdx.x / p.n_img; img = blockIdx.x - tile * p.n_img; }
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const int v = ty * kRectTileH + (int)(threadIdx.x >> 5);
    const int u0 = tx * kRectTileW + (int)(threadIdx.x & 31) * kRectPx;
    if (v >= p.Hd || u0 >= p.Wd) return;

    const float* r = p.records + (size_t)img * S2M2_RECTIFY_RECORD_FLOATS;             // block-uniform
    int s = (int)r[S2M2_RECTIFY_REC_SRC];
    s = min(max(s, 0), p.n_src - 1);
    const void* src = s ? p.src[1] : p.src[0];
    const float* iR = r + S2M2_RECTIFY_REC_IR;
    const float fx = r[S2M2_RECTIFY_REC_FX], fy = r[S2M2_RECTIFY_REC_FY], cx = r[S2M2_RECTIFY_REC_CX], cy = r[S2M2_RECTIFY_REC_CY];
    const float k1 = r[S2M2_RECTIFY_REC_K1], k2 = r[S2M2_RECTIFY_REC_K2], p1 = r[S2M2_RECTIFY_REC_P1], p2 = r[S2M2_RECTIFY_REC_P2];
    const float k3 = r[S2M2_RECTIFY_REC_K3];

    const float fv = (float)v;
    const float Xr = iR[1] * fv + iR[2], Yr = iR[4] * fv + iR[5], Wr = iR[7] * fv + iR[8];
    float mx[kRectPx], my[kRectPx], val[3][kRectPx];
#pragma unroll
    for (int j = 0; j < kRectPx; ++j) {
        const float fu = (float)(u0 + j);
        const float X = iR[0] * fu + Xr, Y = iR[3] * fu + Yr, W = iR[6] * fu + Wr;
        const float x = X / W, y = Y / W;
        const float x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.f * x * y;
        const float kr = 1.f + ((k3 * r2 + k2) * r2 + k1) * r2;
        const float xd = x * kr + p1 * xy2 + p2 * (r2 + 2.f * x2);
        const float yd = y * kr + p1 * (r2 + 2.f * y2) + p2 * xy2;
        mx[j] = fx * xd + cx;
        my[j] = fy * yd + cy;
    }
    if (src) {
#pragma unroll
        for (int j = 0; j < kRectPx; ++j) {
            // a footprint that touches the source: floor in [-1, Ws-1] x [-1, Hs-1]; anything else (NaN included) is all border
            const bool touch = mx[j] > -1.f && mx[j] < (float)p.Ws && my[j] > -1.f && my[j] < (float)p.Hs;
            const float flx = touch ? floorf(mx[j]) : 0.f, fly = touch ? floorf(my[j]) : 0.f;
            const float wx = touch ? mx[j] - flx : 0.f, wy = touch ? my[j] - fly : 0.f;
            const int x0 = (int)flx, y0 = (int)fly;
            const bool in_x0 = touch && x0 >= 0, in_x1 = touch && x0 + 1 < p.Ws, in_y0 = y0 >= 0, in_y1 = y0 + 1 < p.Hs;
            const int xa = max(x0, 0), xb = min(x0 + 1, p.Ws - 1), ya = max(y0, 0), yb = min(y0 + 1, p.Hs - 1);
            float t00[3], t01[3], t10[3], t11[3];
            rect_fetch<FMT>(src, p.Hs, p.Ws, ya, xa, t00);
            rect_fetch<FMT>(src, p.Hs, p.Ws, ya, xb, t01);
            rect_fetch<FMT>(src, p.Hs, p.Ws, yb, xa, t10);
            rect_fetch<FMT>(src, p.Hs, p.Ws, yb, xb, t11);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float a = (in_x0 && in_y0) ? t00[c] : 0.f, b = (in_x1 && in_y0) ? t01[c] : 0.f;
                const float d = (in_x0 && in_y1) ? t10[c] : 0.f, e = (in_x1 && in_y1) ? t11[c] : 0.f;
                const float top = a + wx * (b - a), bot = d + wx * (e - d);
                float o = top + wy * (bot - top);
                if (OUT_U8) o = rintf(fminf(fmaxf(o, 0.f), 255.f));
                else if (p.round) o = rintf(o);
                val[c][j] = o;
            }
        }
        const size_t plane = (size_t)p.Hd * p.Wd;
        const size_t at = (size_t)img * 3 * plane + (size_t)v * p.Wd + u0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (OUT_U8) {
                unsigned char* o = static_cast<unsigned char*>(p.out) + at + c * plane;
                if (VEC) {                                   // Wd % 4 == 0: the group is whole and 4-byte aligned
                    uchar4_t q = {(unsigned char)val[c][0], (unsigned char)val[c][1], (unsigned char)val[c][2], (unsigned char)val[c][3]};
                    *reinterpret_cast<uchar4_t*>(o) = q;
                } else {
#pragma unroll
                    for (int j = 0; j < kRectPx; ++j)
                        if (u0 + j < p.Wd) o[j] = (unsigned char)val[c][j];
                }
            } else {
                float* o = static_cast<float*>(p.out) + at + c * plane;
                if (VEC) {
                    float4_t q = {val[c][0], val[c][1], val[c][2], val[c][3]};
                    *reinterpret_cast<float4_t*>(o) = q;
                } else {
#pragma unroll
                    for (int j = 0; j < kRectPx; ++j)
                        if (u0 + j < p.Wd) o[j] = val[c][j];
                }
            }
        }
    }
    if (p.maps) {
        const size_t plane = (size_t)p.Hd * p.Wd;
        float* ox = p.maps + (size_t)img * 2 * plane + (size_t)v * p.Wd + u0;
        float* oy = ox + plane;
        if (VEC) {
            float4_t qx = {mx[0], mx[1], mx[2], mx[3]}, qy = {my[0], my[1], my[2], my[3]};
            *reinterpret_cast<float4_t*>(ox) = qx;
            *reinterpret_cast<float4_t*>(oy) = qy;
        } else {
#pragma unroll
            for (int j = 0; j < kRectPx; ++j)
                if (u0 + j < p.Wd) { ox[j] = mx[j]; oy[j] = my[j]; }
        }
    }
}

template <int FMT, bool OUT_U8> static int rect_launch(const RectParams& p, bool vec, hipStream_t s) {
    const dim3 grid((unsigned)((long long)p.tiles * p.n_img)), block(kRectThreads);
    if (vec) return launch<rectify_kernel<FMT, OUT_U8, true>>("rectify", grid, block, 0, s, p);
    return launch<rectify_kernel<FMT, OUT_U8, false>>("rectify", grid, block, 0, s, p);
}

static int rectify_impl(const s2m2_rectify_desc* d, void* stream) {
    S2M2_REQUIRE(d != nullptr, "rectify: null descriptor");
    S2M2_REQUIRE(!plan_recording(), "rectify: s2m2_rectify is not recorded in launch plans -- call it outside s2m2_plan_begin .. s2m2_plan_end, "
                                    "before s2m2_plan_run / s2m2_engine_run on the same stream");
    S2M2_REQUIRE(d->records != nullptr, "rectify: null pointer (records)");
    S2M2_REQUIRE(d->out || d->maps, "rectify: no output requested (out and maps are both null pointers)");
    S2M2_REQUIRE(d->n_src == 1 || d->n_src == 2, "rectify: n_src must be 1 or 2 (%d): a record's source index is 0 .. n_src-1", d->n_src);
    S2M2_REQUIRE(d->n_img > 0 && d->Hs > 0 && d->Ws > 0 && d->Hd > 0 && d->Wd > 0, "rectify: non-positive extents n_img=%d Hs=%d Ws=%d Hd=%d Wd=%d",
                 d->n_img, d->Hs, d->Ws, d->Hd, d->Wd);
    S2M2_REQUIRE(d->Hs < (1 << 23) && d->Ws < (1 << 23) && d->Hd < (1 << 23) && d->Wd < (1 << 23) && (long long)d->Hs * d->Ws < (1LL << 31),
                 "rectify: extents too large (every extent < 2^23, Hs*Ws < 2^31)");
    S2M2_REQUIRE(d->src_format == S2M2_RECTIFY_SRC_U8_HWC || d->src_format == S2M2_RECTIFY_SRC_U8_CHW || d->src_format == S2M2_RECTIFY_SRC_F32_CHW,
                 "rectify: unsupported source format %d", d->src_format);
    S2M2_REQUIRE(d->out_dtype == S2M2_F32 || d->out_dtype == 2, "rectify: unsupported output dtype %d", d->out_dtype);
    S2M2_REQUIRE(d->order == S2M2_RECTIFY_ORDER_SAMPLE || d->order == S2M2_RECTIFY_ORDER_TILE, "rectify: unknown block order %d", d->order);
    if (d->out) {
        for (int i = 0; i < d->n_src; ++i) {
            S2M2_REQUIRE(d->src[i] != nullptr, "rectify: null pointer (src[%d]) with n_src = %d", i, d->n_src);
            S2M2_REQUIRE(d->src_format != S2M2_RECTIFY_SRC_F32_CHW || ((uintptr_t)d->src[i] & 3) == 0, "rectify: an fp32 source must be 4-byte aligned");
        }
        S2M2_REQUIRE(d->out_dtype != S2M2_F32 || ((uintptr_t)d->out & 3) == 0, "rectify: an fp32 output must be 4-byte aligned");
    }
    S2M2_REQUIRE(((uintptr_t)d->records & 3) == 0 && ((uintptr_t)d->maps & 3) == 0, "rectify: records and maps must be 4-byte aligned");
    const int tiles_x = (d->Wd + kRectTileW - 1) / kRectTileW, tiles_y = (d->Hd + kRectTileH - 1) / kRectTileH;
    S2M2_REQUIRE((long long)tiles_x * tiles_y * d->n_img < (1LL << 31), "rectify: too many blocks (n_img = %d images of %d x %d)", d->n_img, d->Wd, d->Hd);

    RectParams p;
    p.src[0] = d->out ? d->src[0] : nullptr;
    p.src[1] = d->out && d->n_src == 2 ? d->src[1] : p.src[0];
    p.records = d->records; p.out = d->out; p.maps = d->maps;
    p.n_src = d->n_src; p.n_img = d->n_img;
    p.Hs = d->Hs; p.Ws = d->Ws; p.Hd = d->Hd; p.Wd = d->Wd;
    p.tiles_x = tiles_x; p.tiles = tiles_x * tiles_y;
    p.round = d->round != 0; p.tile_fastest = d->order == S2M2_RECTIFY_ORDER_TILE;
    // whole 16-byte (fp32) / 4-byte (uint8) groups: every row starts on a multiple of four elements and the bases are aligned
    const bool u8 = d->out_dtype == 2;
    const bool vec = d->Wd % 4 == 0 && ((uintptr_t)d->out & (u8 ? 3 : 15)) == 0 && ((uintptr_t)d->maps & 15) == 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
#define S2M2_RECT_FMT(F) (u8 ? rect_launch<F, true>(p, vec, s) : rect_launch<F, false>(p, vec, s))
    if (d->src_format == S2M2_RECTIFY_SRC_U8_HWC) return S2M2_RECT_FMT(S2M2_RECTIFY_SRC_U8_HWC);
    if (d->src_format == S2M2_RECTIFY_SRC_U8_CHW) return S2M2_RECT_FMT(S2M2_RECTIFY_SRC_U8_CHW);
    return S2M2_RECT_FMT(S2M2_RECTIFY_SRC_F32_CHW);
#undef S2M2_RECT_FMT
}

}  // namespace s2m2

extern "C" int s2m2_rectify(const s2m2_rectify_desc* desc, void* stream) { return s2m2::rectify_impl(desc, stream); }
