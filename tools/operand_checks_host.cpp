// Stand-alone host check of the operand validators of the fused convolution entry points (csrc/launch.h: check_activation, check_weight_stream,
// check_disjoint): every refused and accepted descriptor of tests/test_convblock_cpu.py, tests/test_conv_gru_cpu.py and tests/test_convtail_cpu.py
// that they decide, and of the host geometry of the raster-order output stages K15 / K18 / K20 (csrc/raster_host.h: extent bounds, padded-map
// checks, tile geometry, workspace rounding) at and just past every bound, as plain calls -- host code only, no device, no library.  Meant for
// a sanitizer build:
//
//     hipcc --offload-host-only -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all tools/operand_checks_host.cpp -o operand_checks_host
//     ./operand_checks_host        (prints "ok: N checks", exit status 0)
#include "../s2m2_amd/csrc/launch.h"
#include "../s2m2_amd/csrc/raster_host.h"

#include <string.h>

static char g_msg[512];
namespace s2m2 {
int set_error(const char* fmt, ...) {           // the library's is in runtime.hip; this program links nothing of it
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    return 1;
}
}  // namespace s2m2

static int g_checks = 0, g_failed = 0;
// rc != 0 and the message contains `want`; want == nullptr: accepted
static void expect(int rc, const char* want, int line) {
    ++g_checks;
    const bool ok = want ? (rc != 0 && strstr(g_msg, want) != nullptr) : rc == 0;
    if (!ok) {
        ++g_failed;
        fprintf(stderr, "line %d: rc=%d message \"%s\", expected %s%s\n", line, rc, rc ? g_msg : "", want ? "a refusal with " : "acceptance", want ? want : "");
    }
    g_msg[0] = 0;
}
#define EXPECT(call, want) expect((call), (want), __LINE__)
// a value of the host geometry
#define CHECK(cond)                                                   \
    do {                                                              \
        ++g_checks;                                                   \
        if (!(cond)) {                                                \
            ++g_failed;                                               \
            fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
        }                                                             \
    } while (0)

int main() {
    using namespace s2m2;
    const auto P = [](unsigned long long a) { return reinterpret_cast<const void*>(a); };   // addresses are compared, never followed
    const unsigned long long A = 1ull << 20, B = 2ull << 20;
    const int C = 128;
    const long long px = 4 * 40, span = px * C * 2;               // one 4 x 40 x 128 fp16 tensor

    // activation tensors
    EXPECT(check_activation("conv_block", "x", P(A), C, px, C), nullptr);
    EXPECT(check_activation("conv_block", "x", P(A), 136, px, C), nullptr);
    EXPECT(check_activation("conv_block", "x", nullptr, C, px, C), "conv_block: x is null");
    EXPECT(check_activation("conv_block", "x", P(A + 4), C, px, C), "conv_block: x must be 16-byte aligned");
    EXPECT(check_activation("conv_block", "x", P(A + 8), C, px, C), "x must be 16-byte aligned");
    EXPECT(check_activation("conv_block", "x", P(A), 120, px, C), "x_stride=120 (at least C = 128 and a multiple of 8)");
    EXPECT(check_activation("conv_block", "x", P(A), 132, px, C), "x_stride=132");
    EXPECT(check_activation("conv_block", "out", P(B + 8), 132, px, C, 8), nullptr);              // K14's out: 8-byte stores
    EXPECT(check_activation("conv_block", "out", P(B + 4), C, px, C, 8), "out must be 8-byte aligned");
    EXPECT(check_activation("conv_block", "out", P(B), 130, px, C, 8), "out_stride=130 (at least C = 128 and a multiple of 4)");
    EXPECT(check_activation("conv_block", "out", nullptr, C, px, C, 8), "out is null");
    EXPECT(check_activation("conv_gru", "h", P(A), 120, px, C), "conv_gru: h_stride=120");
    EXPECT(check_activation("conv_gru", "out", P(A), 64, px, C), "out_stride=64");
    // 32-bit offsets (K19): 2^22 pixels at a stride of 2^10 elements; the kernels that index with long long take the same tensor
    EXPECT(check_activation("conv_block_tail", "z", P(A), 1 << 10, 1LL << 22, C, 16, true), "conv_block_tail: z spans 2^31 elements or more");
    EXPECT(check_activation("conv_block_tail", "z", P(A), 1 << 9, (1LL << 22) - 1, C, 16, true), nullptr);
    EXPECT(check_activation("conv_gru", "x", P(A), 1 << 10, 1LL << 22, C), nullptr);

    // weight streams
    EXPECT(check_weight_stream("conv_block", "w_conv0", P(4096)), nullptr);
    EXPECT(check_weight_stream("conv_block", "w_1x2", nullptr), "conv_block: w_1x2 is null");
    EXPECT(check_weight_stream("conv_gru", "w_q", nullptr), "conv_gru: w_q is null");
    EXPECT(check_weight_stream("conv_block", "w_1x0", P(4100)), "w_1x0 must be 16-byte aligned");

    // byte ranges of out and one input
    EXPECT(check_disjoint("conv_block", "x", P(A), C, P(B), C, px, C), nullptr);
    EXPECT(check_disjoint("conv_block", "x", P(A), C, P(A), C, px, C), "conv_block: out aliases x");
    EXPECT(check_disjoint("conv_block", "x", P(A), C, P(A + span - 16), C, px, C), "out aliases x");      // out starts on the last 16 bytes of x
    EXPECT(check_disjoint("conv_block", "x", P(A), C, P(A - span + 16), C, px, C), "out aliases x");      // out ends 16 bytes into x
    EXPECT(check_disjoint("conv_block", "x", P(A), C, P(A + span), C, px, C), nullptr);                   // back to back
    EXPECT(check_disjoint("conv_block", "x", P(A), C, P(A - span), C, px, C), nullptr);
    EXPECT(check_disjoint("conv_gru", "h", P(A), C, P(A + span - 16), C, px, C), "conv_gru: out aliases h");
    EXPECT(check_disjoint("conv_gru", "x", P(B), C, P(B - span + 16), C, px, C), "conv_gru: out aliases x");
    // strided operands: x as a channel slice of a 136-channel tensor, out inside the same allocation's unused channels still overlaps in bytes
    EXPECT(check_disjoint("conv_block", "x", P(A + 16), 136, P(A), 136, px, C), "out aliases x");
    EXPECT(check_disjoint("conv_block_tail", "t", P(A), 3 * C, P(B), C + 64, px, C), nullptr);
    EXPECT(check_disjoint("conv_block", "x", P(A), C, P(B), C, 1, C), nullptr);                           // one pixel

    // raster-order output stages: extents at and just past every bound
    const int M = 0x7fffffff;                                                                     // 2^31 - 1
    CHECK(raster_extents_ok(1, 1, 1) && raster_extents_ok(65535, 1, 1) && !raster_extents_ok(65536, 1, 1));
    CHECK(!raster_extents_ok(0, 1, 1) && !raster_extents_ok(1, 0, 1) && !raster_extents_ok(1, 1, 0) && !raster_extents_ok(-1, 1, 1) && !raster_extents_ok(1, -4, -4));
    CHECK(raster_extents_ok(1, 1, M) && raster_extents_ok(1, M, 1) && !raster_extents_ok(1, 2, 1 << 30) && !raster_extents_ok(1, 1 << 16, 1 << 15));
    CHECK(raster_extents_ok(1, 46340, 46340) && !raster_extents_ok(1, M, M));                     // (no 32-bit product)
    CHECK(raster_extents_ok(1, 1, (1 << 30) - 1, 1LL << 30) && !raster_extents_ok(1, 1, 1 << 30, 1LL << 30) && !raster_extents_ok(1, 1 << 15, 1 << 15, 1LL << 30));   // K20
    CHECK(raster_extents_ok(65535, 32767, 32768, 1LL << 30) && !raster_extents_ok(65536, 1, 1, 1LL << 30));
    EXPECT(check_padded_maps("cloud", "image", 1, 1000, 1190, 1024, 1216), nullptr);
    EXPECT(check_padded_maps("cloud", "image", 65535, 1, 1, 1, 1), nullptr);
    EXPECT(check_padded_maps("cloud", "image", 1, 1, M, 1, M), nullptr);
    EXPECT(check_padded_maps("mesh", "image", 0, 4, 4, 4, 4), "mesh: non-positive extents B=0 H=4 W=4 Hp=4 Wp=4");
    EXPECT(check_padded_maps("cloud", "image", 1, 4, 4, 4, -4), "cloud: non-positive extents B=1 H=4 W=4 Hp=4 Wp=-4");
    EXPECT(check_padded_maps("cloud", "image", 1, 5, 4, 4, 4), "cloud: the image (H=5, W=4) is larger than the maps (Hp=4, Wp=4)");
    EXPECT(check_padded_maps("disp_eval", "ground truth", 1, 4, 5, 4, 4), "disp_eval: the ground truth (H=4, W=5) is larger than the maps (Hp=4, Wp=4)");
    EXPECT(check_padded_maps("cloud", "image", 65536, 4, 4, 4, 4), "cloud: extents too large (B <= 65535, H*W < 2^31)");
    EXPECT(check_padded_maps("disp_eval", "ground truth", 1, 2, 1 << 30, 2, 1 << 30), "disp_eval: extents too large (B <= 65535, H*W < 2^31)");
    EXPECT(check_padded_maps("cloud", "image", 1, 4, 4, 1 << 16, 1 << 15), "cloud: extents too large");      // the maps alone: Hp*Wp = 2^31
    EXPECT(check_padded_maps("cloud", "image", 1, 4, 4, M, M), "cloud: extents too large");

    // tile geometry: K15's and K18's 4096 pixels, K20's 2048; K18's cap of 1024 tiles per pair
    for (const int T : {4096, 2048}) {
        CHECK(tile_rows(1, T) == T && tile_rows(2, T) == T / 2 && tile_rows(3, T) == T / 3);
        CHECK(tile_rows(T - 1, T) == 1 && tile_rows(T, T) == 1 && tile_rows(T + 1, T) == 1 && tile_rows(M, T) == 1);
        CHECK(tile_rows(T / 2, T) == 2 && tile_rows(T / 2 + 1, T) == 1);
    }
    CHECK(tile_rows(1216, 4096) == 3 && tile_rows(1216, 2048) == 1 && tile_rows(61, 4096) == 67 && tile_rows(61, 2048) == 33);
    CHECK(tiles(1, 1) == 1 && tiles(1, 4096) == 1 && tiles(4096, 4096) == 1 && tiles(4097, 4096) == 2 && tiles(140, 67) == 3 && tiles(M, 1) == M);
    CHECK(tiles(M, 4096) == (1 << 19) && tiles(M, M) == 1 && tiles(M, 2) == (1 << 30));            // (H + rows - 1 passes 2^31: formed in 64 bits)
    CHECK(round256(0) == 0 && round256(1) == 256 && round256(255) == 256 && round256(256) == 256 && round256(257) == 512);
    CHECK(round256((size_t)65535 * M * 4) == ((size_t)65535 * M * 4 + 255) / 256 * 256);
    CHECK(tile_rows_capped(1024, 1216, 4096, 1024) == 3 && tile_rows_capped(1, 1, 4096, 1024) == 4096);
    CHECK(tile_rows_capped(1024, 4096, 4096, 1024) == 1 && tile_rows_capped(1025, 4096, 4096, 1024) == 2 && tile_rows_capped(2049, 5000, 4096, 1024) == 3);
    CHECK(tile_rows_capped(4096 * 1024, 1, 4096, 1024) == 4096 && tile_rows_capped(4096 * 1024 + 1, 1, 4096, 1024) == 4097);
    CHECK(tile_rows_capped(M, 1, 4096, 1024) == (1 << 21) && tiles(M, tile_rows_capped(M, 1, 4096, 1024)) == 1024);
    for (const int H : {1, 1023, 1024, 1025, 3072, 3073, 100000, M / 4100})                       // never more than the cap, never an empty tile
        for (const int W : {1, 3, 4095, 4096, 4097}) {
            const int rows = tile_rows_capped(H, W, 4096, 1024), n = tiles(H, rows);
            CHECK(rows >= 1 && n >= 1 && n <= 1024 && (long long)(n - 1) * rows < H);
        }

    if (g_failed) {
        fprintf(stderr, "%d of %d checks failed\n", g_failed, g_checks);
        return 1;
    }
    printf("ok: %d checks\n", g_checks);
    return 0;
}
