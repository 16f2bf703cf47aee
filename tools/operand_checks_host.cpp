// Stand-alone host check of the operand validators of the fused convolution entry points (csrc/launch.h: check_activation, check_weight_stream,
// check_disjoint): every refused and accepted descriptor of tests/test_convblock_cpu.py, tests/test_conv_gru_cpu.py and tests/test_convtail_cpu.py
// that they decide, as plain calls -- host code only, no device, no library.  Meant for a sanitizer build:
//
//     hipcc --offload-host-only -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all tools/operand_checks_host.cpp -o operand_checks_host
//     ./operand_checks_host        (prints "ok: N checks", exit status 0)
#include "../s2m2_amd/csrc/launch.h"

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

    if (g_failed) {
        fprintf(stderr, "%d of %d checks failed\n", g_failed, g_checks);
        return 1;
    }
    printf("ok: %d checks\n", g_checks);
    return 0;
}
