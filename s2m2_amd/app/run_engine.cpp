// s2m2_run_engine: runs an engine file (s2m2_amd/export.py: export_engine) with nothing but libs2m2_hip.so and the HIP runtime.
//
//   s2m2_run_engine ENGINE LEFT RIGHT [--out DIR] [--repeat N]
//
// LEFT / RIGHT: raw little-endian float32 (B,3,H,W) images in [0,255], the engine's B, H and W (the engine must take float32 images).
// --out DIR: writes DIR/disp.f32, DIR/occ.f32, DIR/conf.f32, each a raw float32 (B,1,out_h,out_w) map.
// --repeat N: after the run above and a warm-up, N more runs timed with HIP events around them; prints the milliseconds per pair.
//
// 3D outputs (s2m2_cloud on the device buffers of the run; without --calib nothing below happens):
//   --calib FILE [--image LEFT.u8] [--depth-trunc M] [--depth-scale S] [--conf-min X] [--occ-min X] [--unfiltered] --ply OUT.ply [--depth OUT.f32]
// --calib FILE: a Middlebury calib.txt (cam0=[fx 0 cx; 0 fy cy; 0 0 1], doffs=, baseline=), used as it stands (full resolution).
// --image: raw uint8 (B,3,H,W) left image for the colours; without it the colours are the float32 LEFT input, rounded.
// --ply: a binary little-endian PLY (x y z float, red green blue alpha uchar; the device records verbatim).  B > 1: one file per pair,
//   OUT.<b>.ply (a trailing ".ply" of OUT is dropped first).  --depth: raw float32 (B,1,H,W) metric depth, 0 where no point was kept.
// With --repeat the cloud stage is timed as well (HIP events around N calls) and its microseconds per pair printed on a line of its own.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "s2m2_hip.h"

static const char* USAGE =
    "usage: s2m2_run_engine ENGINE LEFT RIGHT [--out DIR] [--repeat N] [--calib FILE [--image LEFT.u8] [--depth-trunc M] [--depth-scale S] "
    "[--conf-min X] [--occ-min X] [--unfiltered] --ply OUT.ply [--depth OUT.f32]]";

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

// cam0=[fx 0 cx; 0 fy cy; 0 0 1], doffs=, baseline= of a Middlebury calib.txt; every other key is ignored
struct Calib {
    double fx = 0, fy = 0, cx = 0, cy = 0, doffs = 0, baseline = 0;
    bool have_cam0 = false, have_baseline = false;
};

static bool read_calib(const char* path, Calib& c) {
    FILE* f = fopen(path, "r");
    if (!f) return false;
    char line[512];
    while (fgets(line, sizeof line, f)) {
        double m[9];
        if (sscanf(line, " cam0 = [ %lf %lf %lf ; %lf %lf %lf ; %lf %lf %lf", m, m + 1, m + 2, m + 3, m + 4, m + 5, m + 6, m + 7, m + 8) == 9) {
            c.fx = m[0]; c.cx = m[2]; c.fy = m[4]; c.cy = m[5];
            c.have_cam0 = true;
        } else if (sscanf(line, " doffs = %lf", m) == 1) c.doffs = m[0];
        else if (sscanf(line, " baseline = %lf", m) == 1) { c.baseline = m[0]; c.have_baseline = true; }
    }
    fclose(f);
    return c.have_cam0 && c.have_baseline;
}

static bool write_ply(const std::string& path, const void* records, long long n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %lld\nproperty float x\nproperty float y\nproperty float z\n"
               "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n", n);
    const bool ok = fwrite(records, 16, (size_t)n, f) == (size_t)n;
    return fclose(f) == 0 && ok;
}

#define HIP_OK(x, what)                              \
    do {                                             \
        if ((x) != hipSuccess) return fail(what);    \
    } while (0)

int main(int argc, char** argv) {
    const char* pos[3] = {nullptr, nullptr, nullptr};
    const char* out_dir = nullptr;
    const char *calib_path = nullptr, *image_path = nullptr, *ply_path = nullptr, *depth_path = nullptr;
    double depth_trunc = 0.0, depth_scale = 1000.0, conf_min = 0.1, occ_min = 0.5;
    int unfiltered = 0;
    int repeat = 0, npos = 0;
    for (int i = 1; i < argc; ++i) {
        if (strcmp(argv[i], "--out") == 0 && i + 1 < argc) out_dir = argv[++i];
        else if (strcmp(argv[i], "--calib") == 0 && i + 1 < argc) calib_path = argv[++i];
        else if (strcmp(argv[i], "--image") == 0 && i + 1 < argc) image_path = argv[++i];
        else if (strcmp(argv[i], "--ply") == 0 && i + 1 < argc) ply_path = argv[++i];
        else if (strcmp(argv[i], "--depth") == 0 && i + 1 < argc) depth_path = argv[++i];
        else if (strcmp(argv[i], "--depth-trunc") == 0 && i + 1 < argc) depth_trunc = atof(argv[++i]);
        else if (strcmp(argv[i], "--depth-scale") == 0 && i + 1 < argc) depth_scale = atof(argv[++i]);
        else if (strcmp(argv[i], "--conf-min") == 0 && i + 1 < argc) conf_min = atof(argv[++i]);
        else if (strcmp(argv[i], "--occ-min") == 0 && i + 1 < argc) occ_min = atof(argv[++i]);
        else if (strcmp(argv[i], "--unfiltered") == 0) unfiltered = 1;
        else if (strcmp(argv[i], "--repeat") == 0 && i + 1 < argc) repeat = atoi(argv[++i]);
        else if (npos < 3 && argv[i][0] != '-') pos[npos++] = argv[i];
        else return fail(USAGE);
    }
    if (npos != 3 || repeat < 0) return fail(USAGE);
    if ((calib_path == nullptr) != (ply_path == nullptr)) return fail("--calib and --ply come together");
    if (!calib_path && (image_path || depth_path)) return fail("--image and --depth need --calib and --ply");
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
    if (calib_path) {
        Calib cal;
        if (!read_calib(calib_path, cal)) return fail("--calib: cannot read cam0 and baseline from the file");
        if (m.out_h != m.H || m.out_w != m.W) return fail("the 3D outputs need maps of the image's size (an engine without output_upsample)");
        const size_t npix = (size_t)m.H * m.W;
        void *dimg = nullptr, *drec = nullptr, *dws = nullptr;
        int32_t* dcount = nullptr;
        float* ddepth = nullptr;
        if (image_path) {
            std::vector<unsigned char> hi(img);
            FILE* f = fopen(image_path, "rb");
            const bool ok = f && fread(hi.data(), 1, img, f) == img && fgetc(f) == EOF;
            if (f) fclose(f);
            if (!ok) {
                fprintf(stderr, "s2m2_run_engine: --image must be a raw uint8 (%d,3,%d,%d) file\n", m.B, m.H, m.W);
                return 1;
            }
            HIP_OK(hipMalloc(&dimg, img), "hipMalloc");
            HIP_OK(hipMemcpy(dimg, hi.data(), img, hipMemcpyHostToDevice), "upload");
        }
        const size_t ws_bytes = s2m2_cloud_workspace_bytes(m.B, m.H, m.W);
        HIP_OK(hipMalloc(&drec, (size_t)m.B * npix * 16), "hipMalloc");
        HIP_OK(hipMalloc(&dws, ws_bytes), "hipMalloc");
        HIP_OK(hipMalloc((void**)&dcount, m.B * sizeof(int32_t)), "hipMalloc");
        if (depth_path) HIP_OK(hipMalloc((void**)&ddepth, (size_t)m.B * npix * sizeof(float)), "hipMalloc");
        s2m2_cloud_desc cd;
        memset(&cd, 0, sizeof cd);
        cd.disp = dout[0]; cd.occ = dout[1]; cd.conf = dout[2];
        cd.image = image_path ? dimg : dl;
        cd.image_dtype = image_path ? 2 : S2M2_F32;
        cd.depth = ddepth; cd.records = drec; cd.count = dcount; cd.workspace = dws;
        cd.B = m.B; cd.H = m.H; cd.W = m.W; cd.Hp = m.out_h; cd.Wp = m.out_w;
        cd.unfiltered = unfiltered;
        cd.capacity = (long long)npix;
        cd.fx = cal.fx; cd.fy = cal.fy; cd.cx = cal.cx; cd.cy = cal.cy; cd.baseline = cal.baseline; cd.doffs = cal.doffs;
        cd.depth_scale = depth_scale; cd.depth_trunc = depth_trunc; cd.conf_min = conf_min; cd.occ_min = occ_min;
        if (s2m2_cloud(&cd, s) != 0) return fail_lib("s2m2_cloud failed");
        HIP_OK(hipStreamSynchronize(s), "s2m2_cloud");
        std::vector<int32_t> hcount(m.B);
        HIP_OK(hipMemcpy(hcount.data(), dcount, m.B * sizeof(int32_t), hipMemcpyDeviceToHost), "download");
        std::string stem = ply_path;
        if (m.B > 1 && stem.size() > 4 && stem.compare(stem.size() - 4, 4, ".ply") == 0) stem.resize(stem.size() - 4);
        std::vector<unsigned char> hrec;
        for (int b = 0; b < m.B; ++b) {
            hrec.resize((size_t)hcount[b] * 16);
            HIP_OK(hipMemcpy(hrec.data(), (const char*)drec + (size_t)b * npix * 16, hrec.size(), hipMemcpyDeviceToHost), "download");
            const std::string path = m.B > 1 ? stem + "." + std::to_string(b) + ".ply" : stem;
            if (!write_ply(path, hrec.data(), hcount[b])) return fail("cannot write the PLY file");
        }
        if (depth_path) {
            std::vector<float> hd((size_t)m.B * npix);
            HIP_OK(hipMemcpy(hd.data(), ddepth, hd.size() * sizeof(float), hipMemcpyDeviceToHost), "download");
            if (!write_raw(depth_path, hd)) return fail("cannot write the depth map");
        }
        if (repeat > 0) {
            hipEvent_t t0, t1;
            HIP_OK(hipEventCreate(&t0), "hipEventCreate");
            HIP_OK(hipEventCreate(&t1), "hipEventCreate");
            HIP_OK(hipEventRecord(t0, s), "hipEventRecord");
            for (int i = 0; i < repeat; ++i)
                if (s2m2_cloud(&cd, s) != 0) return fail_lib("s2m2_cloud failed");
            HIP_OK(hipEventRecord(t1, s), "hipEventRecord");
            HIP_OK(hipEventSynchronize(t1), "timed cloud runs");
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, t0, t1), "hipEventElapsedTime");
            printf("{\"cloud_points\": %d, \"repeat\": %d, \"cloud_us_per_pair\": %.2f}\n", hcount[0], repeat, 1000.f * ms / repeat / m.B);
            (void)hipEventDestroy(t0);
            (void)hipEventDestroy(t1);
        }
        (void)hipFree(dimg);
        (void)hipFree(drec);
        (void)hipFree(dws);
        (void)hipFree(dcount);
        (void)hipFree(ddepth);
    }
    s2m2_engine_destroy(eng);
    for (auto& p : dout) (void)hipFree(p);
    (void)hipFree(dl);
    (void)hipFree(dr);
    (void)hipStreamDestroy(s);
    return 0;
}
