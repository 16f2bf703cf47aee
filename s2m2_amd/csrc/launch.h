// Host-side launch helpers shared by every .hip of the library: one launch, one way to read a switch, one dtype dispatch.
#pragma once
#include "common.h"

#include <stdlib.h>

namespace s2m2 {

// Launches Kern (a __global__ function or one instantiation of a __global__ template).  With dynamic LDS it first raises the kernel's limit on the
// current device (reserve_lds: once per size, growing); the per-device "granted" cache is a static of this template, i.e. one per kernel
// instantiation.  `what` prefixes the error text.
template <auto Kern, typename... A>
static int launch(const char* what, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const A&... args) {
    if (lds_bytes) {
        static size_t granted[kMaxDevices] = {};
        if (reserve_lds(reinterpret_cast<const void*>(Kern), lds_bytes, granted, what)) return 1;
    }
    hipLaunchKernelGGL(Kern, grid, block, lds_bytes, st, args...);
    return check_launch(what);
}

// Environment switches.  Callers keep each one in a function-local `static const`: read once per process.
static inline long long env_int(const char* name, long long dflt) {       // integer with a default
    const char* e = getenv(name);
    return e ? atoll(e) : dflt;
}
static inline bool env_flag(const char* name) { return getenv(name) != nullptr; }      // "set at all"
static inline bool env_is0(const char* name) { return env_int(name, 1) == 0; }         // "set and equal to 0" (switches a default-on path off)

// Calls f with a value of the element type `dtype` names: by_dtype(dtype, "tanh", [&](auto t) { using T = decltype(t); ... }).
template <typename F>
static int by_dtype(int dtype, const char* what, F&& f) {
    if (dtype == S2M2_F16) return f(half_t{});
    if (dtype == S2M2_F32) return f(float{});
    return set_error("%s: unsupported dtype %d", what, dtype);
}

// The same for an image: S2M2_F32 / S2M2_F16 / 2 = uint8
template <typename F>
static int by_image_dtype(int dtype, const char* what, F&& f) {
    if (dtype == S2M2_F32) return f(float{});
    if (dtype == S2M2_F16) return f(half_t{});
    if (dtype == 2) return f((unsigned char)0);
    return set_error("%s: unsupported image dtype %d", what, dtype);
}

// a.zero = the current device's zero page, or "<what>: cannot allocate the zero page"
template <typename Args>
static int bind_zero_page(Args& a, const char* what) {
    a.zero = zero_page();
    S2M2_REQUIRE(a.zero, "%s: cannot allocate the zero page", what);
    return 0;
}

// One validator per operand kind of the fused convolution entry points (K14, K17, K19): the C ABI is their boundary, engine files reach it with
// no binding in front.  `entry` prefixes the message: "<entry>: <operand> ...".
// An activation tensor of `pixels` pixels x C fp16 channels, `stride` elements from pixel to pixel: non-null; `align`-byte aligned with a pixel
// stride that keeps every pixel so (16 for what the kernel moves in 16-byte pieces, 8 for K14's 8-byte stores); with offsets32, a span below
// 2^31 elements (the kernel indexes it with 32-bit offsets).
static inline int check_activation(const char* entry, const char* name, const void* ptr, long long stride, long long pixels, int C, int align = 16,
                                   bool offsets32 = false) {
    S2M2_REQUIRE(ptr, "%s: %s is null", entry, name);
    S2M2_REQUIRE((uintptr_t)ptr % align == 0, "%s: %s must be %d-byte aligned", entry, name, align);
    S2M2_REQUIRE(stride >= C && stride % (align / 2) == 0, "%s: %s_stride=%lld (at least C = %d and a multiple of %d)", entry, name, stride, C, align / 2);
    S2M2_REQUIRE(!offsets32 || pixels * stride < (1LL << 31), "%s: %s spans 2^31 elements or more", entry, name);
    return 0;
}
// A weight fragment stream: read in 16-byte pieces
static inline int check_weight_stream(const char* entry, const char* name, const void* ptr) {
    S2M2_REQUIRE(ptr, "%s: %s is null", entry, name);
    S2M2_REQUIRE((uintptr_t)ptr % 16 == 0, "%s: %s must be 16-byte aligned", entry, name);
    return 0;
}
// out shares no byte with the input `name`: a block reads halo pixels of the input that another block's patch covers, so even a partial overlap
// is a race between blocks
static inline int check_disjoint(const char* entry, const char* name, const void* in, long long in_stride, const void* out, long long out_stride,
                                 long long pixels, int C) {
    const uintptr_t a0 = (uintptr_t)in, a1 = a0 + (size_t)((pixels - 1) * in_stride + C) * 2;
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (size_t)((pixels - 1) * out_stride + C) * 2;
    S2M2_REQUIRE(o1 <= a0 || a1 <= o0, "%s: out aliases %s", entry, name);
    return 0;
}

}  // namespace s2m2
