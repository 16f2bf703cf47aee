// s2m2_run_engine: runs an engine file (s2m2_amd/export.py: export_engine) with nothing but libs2m2_hip.so and the HIP runtime.
//
//   s2m2_run_engine ENGINE LEFT RIGHT [--out DIR] [--repeat N]
//
// LEFT / RIGHT: raw little-endian float32 (B,3,H,W) images in [0,255], the engine's B, H and W (the engine must take float32 images).
// --out DIR: writes DIR/disp.f32, DIR/occ.f32, DIR/conf.f32, each a raw float32 (B,1,out_h,out_w) map.
// --repeat N: after the run above and a warm-up, N more runs timed with HIP events around them; prints the milliseconds per pair.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "s2m2_hip.h"

static int fail(const char* what) {
    fprintf(stderr, "s2m2_run_engine: %s\n", what);
    return 1;
}

static int fail_lib(const char* what) {
    fprintf(stderr, "s2m2_run_engine: %s: %s\n", what, s2m2_last_error());
    return 1;
}

static bool read_raw(const char* path, std::vector<float>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t n = fread(v.data(), sizeof(float), v.size(), f);
    const bool at_end = fgetc(f) == EOF;
    fclose(f);
    return n == v.size() && at_end;
}

static bool write_raw(const std::string& path, const std::vector<float>& v) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
    return fclose(f) == 0 && ok;
}

#define HIP_OK(x, what)                              \
    do {                                             \
        if ((x) != hipSuccess) return fail(what);    \
    } while (0)

int main(int argc, char** argv) {
    const char* pos[3] = {nullptr, nullptr, nullptr};
    const char* out_dir = nullptr;
    int repeat = 0, npos = 0;
    for (int i = 1; i < argc; ++i) {
        if (strcmp(argv[i], "--out") == 0 && i + 1 < argc) out_dir = argv[++i];
        else if (strcmp(argv[i], "--repeat") == 0 && i + 1 < argc) repeat = atoi(argv[++i]);
        else if (npos < 3 && argv[i][0] != '-') pos[npos++] = argv[i];
        else return fail("usage: s2m2_run_engine ENGINE LEFT RIGHT [--out DIR] [--repeat N]");
    }
    if (npos != 3 || repeat < 0) return fail("usage: s2m2_run_engine ENGINE LEFT RIGHT [--out DIR] [--repeat N]");
    if (s2m2_version() != S2M2_ABI_VERSION) return fail("libs2m2_hip.so was built from another ABI version than this program");

    s2m2_engine* eng = nullptr;
    if (s2m2_engine_load(pos[0], &eng) != 0) return fail_lib("cannot load the engine");
    s2m2_engine_info m;
    s2m2_engine_meta(eng, &m);
    if (m.image_dtype != S2M2_F32) return fail("this program feeds float32 images; the engine takes another image dtype");
    const size_t img = (size_t)m.B * 3 * m.H * m.W, map = (size_t)m.B * m.out_h * m.out_w;
    std::vector<float> hl(img), hr(img);
    if (!read_raw(pos[1], hl) || !read_raw(pos[2], hr)) {
        fprintf(stderr, "s2m2_run_engine: the images must be raw float32 (%d,3,%d,%d) files\n", m.B, m.H, m.W);
        return 1;
    }
    void *dl = nullptr, *dr = nullptr;
    float* dout[3] = {nullptr, nullptr, nullptr};
    HIP_OK(hipMalloc(&dl, img * sizeof(float)), "hipMalloc");
    HIP_OK(hipMalloc(&dr, img * sizeof(float)), "hipMalloc");
    for (auto& p : dout) HIP_OK(hipMalloc(&p, map * sizeof(float)), "hipMalloc");
    HIP_OK(hipMemcpy(dl, hl.data(), img * sizeof(float), hipMemcpyHostToDevice), "upload");
    HIP_OK(hipMemcpy(dr, hr.data(), img * sizeof(float), hipMemcpyHostToDevice), "upload");
    hipStream_t s;
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");

    if (s2m2_engine_run(eng, dl, dr, dout[0], dout[1], dout[2], s) != 0) return fail_lib("engine run failed");
    HIP_OK(hipStreamSynchronize(s), "engine run");
    if (out_dir) {
        const char* names[3] = {"disp.f32", "occ.f32", "conf.f32"};
        std::vector<float> h(map);
        for (int k = 0; k < 3; ++k) {
            HIP_OK(hipMemcpy(h.data(), dout[k], map * sizeof(float), hipMemcpyDeviceToHost), "download");
            if (!write_raw(std::string(out_dir) + "/" + names[k], h)) return fail("cannot write the outputs");
        }
    }
    if (repeat > 0) {
        for (int i = 0; i < 3; ++i)                                  // warm-up: the second run captures the graph
            if (s2m2_engine_run(eng, dl, dr, dout[0], dout[1], dout[2], s) != 0) return fail_lib("engine run failed");
        hipEvent_t t0, t1;
        HIP_OK(hipEventCreate(&t0), "hipEventCreate");
        HIP_OK(hipEventCreate(&t1), "hipEventCreate");
        HIP_OK(hipStreamSynchronize(s), "warm-up");
        HIP_OK(hipEventRecord(t0, s), "hipEventRecord");
        for (int i = 0; i < repeat; ++i)
            if (s2m2_engine_run(eng, dl, dr, dout[0], dout[1], dout[2], s) != 0) return fail_lib("engine run failed");
        HIP_OK(hipEventRecord(t1, s), "hipEventRecord");
        HIP_OK(hipEventSynchronize(t1), "timed runs");
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, t0, t1), "hipEventElapsedTime");
        printf("{\"B\": %d, \"H\": %d, \"W\": %d, \"repeat\": %d, \"ms_per_pair\": %.4f}\n", m.B, m.H, m.W, repeat, ms / repeat / m.B);
        (void)hipEventDestroy(t0);
        (void)hipEventDestroy(t1);
    }
    s2m2_engine_destroy(eng);
    for (auto& p : dout) (void)hipFree(p);
    (void)hipFree(dl);
    (void)hipFree(dr);
    (void)hipStreamDestroy(s);
    return 0;
}
