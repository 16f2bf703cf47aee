// s2m2_run_engine: runs an engine file (s2m2_amd/export.py: export_engine) with nothing but libs2m2_hip.so and the HIP runtime.
//
//   s2m2_run_engine ENGINE LEFT RIGHT [--out DIR] [--repeat N] [3D outputs] [evaluation]
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
// --mesh OUT.ply [--max-jump X]: the surface mesh (s2m2_mesh) -- the same vertices plus "element face" / "property list uchar int vertex_indices":
//   the triangles between neighbouring kept pixels whose disparities differ by at most X px (default 1; "inf": every kept neighbour).  Needs
//   --calib, honours every option above, names its files like --ply for B > 1, and may be given next to --ply or instead of it.  With
//   --repeat: {"mesh_vertices", "mesh_faces", "repeat", "mesh_us_per_pair"} on a line of its own.
//
// --register CAM [--splat N] --register-depth OUT.f32 [--register-image OUT.ppm] [--register-index OUT.i32]: the depth map registered to a second
//   camera (s2m2_register), behind --calib; honours --image, --depth-trunc, --depth-scale, --conf-min, --occ-min and --unfiltered, and may be
//   given next to --ply / --mesh or without them.  CAM is the word "right" (cam1 of --calib at the engine's image size, no rotation, t =
//   (-baseline / depth_scale, 0, 0)) or a text file in the calib file's syntax: width=, height=, cam=[fx 0 cx; 0 fy cy; 0 0 1], R=[r00 r01 r02;
//   r10 r11 r12; r20 r21 r22] (source camera -> target camera; default: the identity), t=[tx ty tz] (in the unit of z; default: 0).
//   --splat: the footprint, 1..4 (default 2).  --register-depth: raw float32 (Ht,Wt) z in the target camera, 0 = hole; --register-index: raw
//   int32 (Ht,Wt) winning source pixel v * W + u, -1 = hole; --register-image: a binary PPM (P6) of the winners' colours.  B > 1: one file per
//   pair each, named as --ply names its files (OUT.<b>.f32, OUT.<b>.i32, OUT.<b>.ppm).  With --repeat: {"register_covered", "repeat", "register_us_per_pair"} on a line
//   of its own.
//
// --min-size N [--max-jump X] [--labels OUT.i32] [--segment-mask OUT.u8]: the speckle filter (s2m2_segment) behind the forward and in front of
//   every 3D output above: the 4-connected components of the kept pixels whose neighbouring disparities differ by at most X px (the --max-jump
//   of --mesh, default 1), and the disparity map without the components of fewer than N pixels (N >= 1; 1 removes nothing).  Needs --calib;
//   honours --depth-trunc, --depth-scale, --conf-min, --occ-min and --unfiltered.  --ply, --mesh, --depth and --register* then read the
//   filtered map with the filter already applied (unfiltered = 1).  --labels: raw int32 (B,1,H,W), the first raster index of every kept pixel's
//   component, -1 = not kept; --segment-mask: raw uint8 (B,1,H,W), 1 = survives.  With --repeat: {"segment_kept", "segment_components",
//   "segment_surviving", "repeat", "segment_us_per_pair"} on a line of its own.  Without --min-size nothing here happens.
//
// Evaluation against ground truth (s2m2_disp_eval on the device buffers of the run; without --gt nothing below happens):
//   --gt FILE.pfm [--gt-region FILE.u8] [--gt-min X] [--thresholds a,b,c] [--conf-min X] [--occ-min X] --metrics OUT.json
// --gt: a greyscale PFM (Pf) of W x (B * H) pixels, H <= out_h and W <= out_w of the engine: the ground truths of the B pairs stacked top to
//   bottom, pair 0 first (B = 1: the file as a benchmark ships it).  A ground truth smaller than the maps is the centred window image_crop cuts.
// --gt-region: raw uint8 (B,1,H,W), a pixel is evaluated where the byte is not 0 (a benchmark's non-occluded mask).
// --gt-min X: ground truth is valid where it is finite and > X (default 0; "-inf": every finite value).  --thresholds: up to 8 bad-pixel
//   thresholds in px, increasing (default 0.5,1,2,4).  --conf-min / --occ-min: the kept set, as for the cloud.
// --metrics: JSON -- {"thresholds": [...], "pairs": [{"words": [the S2M2_EVAL_WORDS raw stat words], n_region, n_eval, nonfinite, epe, rmse, d1,
//   bad_<t>, a50, a90, a95, a99, density, "kept": {the same after the filter}}, ...]}; a ratio of an empty set (0 / 0) or an infinite quantile
//   is written as null.  The ground-truth files are parsed before the engine is loaded; their extents are compared with the engine's right after.
// With --repeat the stage is timed (HIP events around N calls) and its microseconds per pair printed on a line of its own.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "s2m2_hip.h"

static const char* USAGE =
    "usage: s2m2_run_engine ENGINE LEFT RIGHT [--out DIR] [--repeat N] [--calib FILE [--image LEFT.u8] [--depth-trunc M] [--depth-scale S] "
    "[--conf-min X] [--occ-min X] [--unfiltered] [--ply OUT.ply] [--mesh OUT.ply [--max-jump X]] [--depth OUT.f32] "
    "[--register CAM [--splat N] --register-depth OUT.f32 [--register-image OUT.ppm] [--register-index OUT.i32]] "
    "[--min-size N [--labels OUT.i32] [--segment-mask OUT.u8]]] [--gt FILE.pfm [--gt-region FILE.u8] [--gt-min X] "
    "[--thresholds a,b,c] --metrics OUT.json]";

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
    double cam1[4] = {0, 0, 0, 0};      // fx, fy, cx, cy of cam1 (--register right)
    bool have_cam0 = false, have_baseline = false, have_cam1 = false;
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
        } else if (sscanf(line, " cam1 = [ %lf %lf %lf ; %lf %lf %lf ; %lf %lf %lf", m, m + 1, m + 2, m + 3, m + 4, m + 5, m + 6, m + 7, m + 8) == 9) {
            c.cam1[0] = m[0]; c.cam1[1] = m[4]; c.cam1[2] = m[2]; c.cam1[3] = m[5];
            c.have_cam1 = true;
        } else if (sscanf(line, " doffs = %lf", m) == 1) c.doffs = m[0];
        else if (sscanf(line, " baseline = %lf", m) == 1) { c.baseline = m[0]; c.have_baseline = true; }
    }
    fclose(f);
    return c.have_cam0 && c.have_baseline;
}

// the target camera of --register: a text file in the calib file's syntax (see the head of this file)
struct TargetCamera {
    int width = 0, height = 0;
    double fx = 0, fy = 0, cx = 0, cy = 0;
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double t[3] = {0, 0, 0};
};

static bool read_camera(const char* path, TargetCamera& c) {
    FILE* f = fopen(path, "r");
    if (!f) return false;
    char line[512];
    bool have_cam = false;
    while (fgets(line, sizeof line, f)) {
        double m[9];
        if (sscanf(line, " cam = [ %lf %lf %lf ; %lf %lf %lf ; %lf %lf %lf", m, m + 1, m + 2, m + 3, m + 4, m + 5, m + 6, m + 7, m + 8) == 9) {
            c.fx = m[0]; c.cx = m[2]; c.fy = m[4]; c.cy = m[5];
            have_cam = true;
        } else if (sscanf(line, " R = [ %lf %lf %lf ; %lf %lf %lf ; %lf %lf %lf", m, m + 1, m + 2, m + 3, m + 4, m + 5, m + 6, m + 7, m + 8) == 9) {
            memcpy(c.R, m, sizeof c.R);
        } else if (sscanf(line, " t = [ %lf %lf %lf", m, m + 1, m + 2) == 3) {
            memcpy(c.t, m, sizeof c.t);
        } else if (sscanf(line, " width = %lf", m) == 1) c.width = (int)m[0];
        else if (sscanf(line, " height = %lf", m) == 1) c.height = (int)m[0];
    }
    fclose(f);
    return have_cam && c.width > 0 && c.height > 0;
}

static bool write_bytes(const std::string& path, const char* head, const void* data, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(head, 1, strlen(head), f) == strlen(head) && fwrite(data, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

static bool write_ply(const std::string& path, const void* records, long long n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %lld\nproperty float x\nproperty float y\nproperty float z\n"
               "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n", n);
    const bool ok = fwrite(records, 16, (size_t)n, f) == (size_t)n;
    return fclose(f) == 0 && ok;
}

// the same vertices, then every face as a count byte (3) and three little-endian int32 vertex indices: 13 bytes
static bool write_ply_mesh(const std::string& path, const void* records, long long n, const int32_t* faces, long long nf) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %lld\nproperty float x\nproperty float y\nproperty float z\n"
               "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face %lld\n"
               "property list uchar int vertex_indices\nend_header\n", n, nf);
    std::vector<unsigned char> disk((size_t)nf * 13);
    for (long long i = 0; i < nf; ++i) {
        disk[(size_t)i * 13] = 3;
        memcpy(&disk[(size_t)i * 13 + 1], faces + i * 3, 12);
    }
    const bool ok = fwrite(records, 16, (size_t)n, f) == (size_t)n && fwrite(disk.data(), 13, (size_t)nf, f) == (size_t)nf;
    return fclose(f) == 0 && ok;
}

// OUT.ply, or OUT.<b>.ply for engines of more than one pair (a trailing ".ply" of OUT is dropped first); --register-image: ".ppm"
static std::string pair_path(const char* out, int B, int b, const char* ext = ".ply") {
    std::string stem = out;
    if (B <= 1) return stem;
    const size_t ne = strlen(ext);
    if (stem.size() > ne && stem.compare(stem.size() - ne, ne, ext) == 0) stem.resize(stem.size() - ne);
    return stem + "." + std::to_string(b) + ext;
}

// greyscale PFM: "Pf", "width height", "scale" (negative: little-endian), then the rows bottom to top -> rows top to bottom
static bool read_pfm(const char* path, std::vector<float>& v, int& width, int& height, const char*& why) {
    FILE* f = fopen(path, "rb");
    why = "cannot open the file";
    if (!f) return false;
    char magic[3] = {0, 0, 0};
    double scale = 0.0;
    bool ok = false;
    why = "not a greyscale PFM (header Pf, width height, scale)";
    if (fscanf(f, "%2s %d %d %lf", magic, &width, &height, &scale) == 4 && strcmp(magic, "Pf") == 0 && fgetc(f) == '\n' && width > 0 &&
        height > 0 && (long long)width * height < (1LL << 31) && scale != 0.0 && scale == scale) {
        why = "the data is not width * height float32 values";
        v.resize((size_t)width * height);
        ok = true;
        for (int y = height - 1; y >= 0 && ok; --y) ok = fread(v.data() + (size_t)y * width, sizeof(float), width, f) == (size_t)width;
        ok = ok && fgetc(f) == EOF;
        if (ok && scale > 0.0) {                                     // big-endian
            unsigned char* p = reinterpret_cast<unsigned char*>(v.data());
            for (size_t i = 0; i < v.size(); ++i, p += 4) {
                const unsigned char a = p[0], b = p[1];
                p[0] = p[3]; p[1] = p[2]; p[2] = b; p[3] = a;
            }
        }
    }
    fclose(f);
    return ok;
}

static void json_number(FILE* f, const char* key, double x, const char* tail) {
    if (isfinite(x)) fprintf(f, "\"%s\": %.17g%s", key, x, tail);
    else fprintf(f, "\"%s\": null%s", key, tail);
}

// the derived numbers of one ALL / KEPT block (s2m2_amd/evaluate.py: EvalStats, the same arithmetic in double)
static void json_block(FILE* f, const unsigned long long* blk, const float* thr, int nthr) {
    const double n = (double)blk[S2M2_EVAL_N_EVAL], fin = (double)(blk[S2M2_EVAL_N_EVAL] - blk[S2M2_EVAL_N_NONFINITE]);
    fprintf(f, "\"n_region\": %llu, \"n_eval\": %llu, \"nonfinite\": %llu, ", blk[S2M2_EVAL_N_REGION], blk[S2M2_EVAL_N_EVAL], blk[S2M2_EVAL_N_NONFINITE]);
    json_number(f, "epe", (double)blk[S2M2_EVAL_SUM_ABS_Q] / 65536.0 / fin, ", ");
    json_number(f, "rmse", sqrt((double)blk[S2M2_EVAL_SUM_SQ_Q] / 4096.0 / fin), ", ");
    for (int t = 0; t < nthr; ++t) {
        char key[32];
        snprintf(key, sizeof key, "bad_%g", (double)thr[t]);
        json_number(f, key, (double)blk[S2M2_EVAL_BAD + t] / n, ", ");
    }
    json_number(f, "d1", (double)blk[S2M2_EVAL_D1_BAD] / n, "");
}

// upper edge in px of the histogram bin where the cumulative count first reaches p * n; inf for the overflow bin, NaN without pixels
static double eval_quantile(const unsigned long long* hist, double p) {
    unsigned long long n = 0, cum = 0;
    for (int i = 0; i < S2M2_EVAL_HIST_BINS; ++i) n += hist[i];
    if (n == 0) return NAN;
    for (int i = 0; i < S2M2_EVAL_HIST_BINS; ++i) {
        cum += hist[i];
        if ((double)cum >= p * (double)n) return i == S2M2_EVAL_HIST_BINS - 1 ? INFINITY : (double)(i + 1) / 64.0;
    }
    return INFINITY;
}

#define HIP_OK(x, what)                              \
    do {                                             \
        if ((x) != hipSuccess) return fail(what);    \
    } while (0)

int main(int argc, char** argv) {
    const char* pos[3] = {nullptr, nullptr, nullptr};
    const char* out_dir = nullptr;
    const char *calib_path = nullptr, *image_path = nullptr, *ply_path = nullptr, *depth_path = nullptr, *mesh_path = nullptr;
    const char* max_jump_arg = nullptr;
    const char *register_cam = nullptr, *reg_depth_path = nullptr, *reg_image_path = nullptr, *reg_index_path = nullptr, *splat_arg = nullptr;
    const char *min_size_arg = nullptr, *labels_path = nullptr, *segmask_path = nullptr;
    long long min_size = 1;
    int splat = 2;
    double max_jump = 1.0;
    double depth_trunc = 0.0, depth_scale = 1000.0, conf_min = 0.1, occ_min = 0.5;
    int unfiltered = 0;
    int repeat = 0, npos = 0;
    const char *gt_path = nullptr, *region_path = nullptr, *metrics_path = nullptr, *thr_arg = nullptr;
    double gt_min = 0.0;
    for (int i = 1; i < argc; ++i) {
        if (strcmp(argv[i], "--out") == 0 && i + 1 < argc) out_dir = argv[++i];
        else if (strcmp(argv[i], "--calib") == 0 && i + 1 < argc) calib_path = argv[++i];
        else if (strcmp(argv[i], "--image") == 0 && i + 1 < argc) image_path = argv[++i];
        else if (strcmp(argv[i], "--ply") == 0 && i + 1 < argc) ply_path = argv[++i];
        else if (strcmp(argv[i], "--mesh") == 0 && i + 1 < argc) mesh_path = argv[++i];
        else if (strcmp(argv[i], "--max-jump") == 0 && i + 1 < argc) max_jump_arg = argv[++i];
        else if (strcmp(argv[i], "--depth") == 0 && i + 1 < argc) depth_path = argv[++i];
        else if (strcmp(argv[i], "--register") == 0 && i + 1 < argc) register_cam = argv[++i];
        else if (strcmp(argv[i], "--splat") == 0 && i + 1 < argc) splat_arg = argv[++i];
        else if (strcmp(argv[i], "--register-depth") == 0 && i + 1 < argc) reg_depth_path = argv[++i];
        else if (strcmp(argv[i], "--register-image") == 0 && i + 1 < argc) reg_image_path = argv[++i];
        else if (strcmp(argv[i], "--register-index") == 0 && i + 1 < argc) reg_index_path = argv[++i];
        else if (strcmp(argv[i], "--min-size") == 0 && i + 1 < argc) min_size_arg = argv[++i];
        else if (strcmp(argv[i], "--labels") == 0 && i + 1 < argc) labels_path = argv[++i];
        else if (strcmp(argv[i], "--segment-mask") == 0 && i + 1 < argc) segmask_path = argv[++i];
        else if (strcmp(argv[i], "--depth-trunc") == 0 && i + 1 < argc) depth_trunc = atof(argv[++i]);
        else if (strcmp(argv[i], "--depth-scale") == 0 && i + 1 < argc) depth_scale = atof(argv[++i]);
        else if (strcmp(argv[i], "--conf-min") == 0 && i + 1 < argc) conf_min = atof(argv[++i]);
        else if (strcmp(argv[i], "--occ-min") == 0 && i + 1 < argc) occ_min = atof(argv[++i]);
        else if (strcmp(argv[i], "--unfiltered") == 0) unfiltered = 1;
        else if (strcmp(argv[i], "--gt") == 0 && i + 1 < argc) gt_path = argv[++i];
        else if (strcmp(argv[i], "--gt-region") == 0 && i + 1 < argc) region_path = argv[++i];
        else if (strcmp(argv[i], "--gt-min") == 0 && i + 1 < argc) gt_min = atof(argv[++i]);
        else if (strcmp(argv[i], "--thresholds") == 0 && i + 1 < argc) thr_arg = argv[++i];
        else if (strcmp(argv[i], "--metrics") == 0 && i + 1 < argc) metrics_path = argv[++i];
        else if (strcmp(argv[i], "--repeat") == 0 && i + 1 < argc) repeat = atoi(argv[++i]);
        else if (npos < 3 && argv[i][0] != '-') pos[npos++] = argv[i];
        else return fail(USAGE);
    }
    if (npos != 3 || repeat < 0) return fail(USAGE);
    if (mesh_path && !calib_path) return fail("--calib and --mesh come together");
    if (register_cam && (!calib_path || !reg_depth_path)) return fail("--register needs --calib and --register-depth");
    if (!register_cam && (reg_depth_path || reg_image_path || reg_index_path || splat_arg)) return fail("--splat and --register-* need --register");
    if (splat_arg) {
        splat = atoi(splat_arg);
        if (splat < 1 || splat > 4) return fail("--splat: 1, 2, 3 or 4");
    }
    if (min_size_arg && !calib_path) return fail("--min-size needs --calib");
    if (!min_size_arg && (labels_path || segmask_path)) return fail("--labels and --segment-mask need --min-size");
    if (min_size_arg) {
        char* end = nullptr;
        min_size = strtoll(min_size_arg, &end, 10);
        if (end == min_size_arg || *end || min_size < 1 || min_size > (1LL << 30)) return fail("--min-size: an integer >= 1 (at most 2^30)");
    }
    if (!mesh_path && !register_cam && !min_size_arg && (calib_path == nullptr) != (ply_path == nullptr)) return fail("--calib and --ply come together");
    if ((register_cam || min_size_arg) && !mesh_path && !ply_path && depth_path) return fail("--depth needs --ply or --mesh");
    if (max_jump_arg && !mesh_path && !min_size_arg) return fail("--max-jump needs --mesh or --min-size");
    if (max_jump_arg) {
        char* end = nullptr;
        max_jump = strtod(max_jump_arg, &end);
        if (end == max_jump_arg || *end || !(max_jump >= 0.0)) return fail("--max-jump: a number >= 0 (inf is allowed)");
    }
    if (!calib_path && (image_path || depth_path)) return fail("--image and --depth need --calib and --ply");
    if ((gt_path == nullptr) != (metrics_path == nullptr)) return fail("--gt and --metrics come together");
    if (!gt_path && (region_path || thr_arg)) return fail("--gt-region and --thresholds need --gt and --metrics");
    // the ground truth is parsed and validated here, before the engine is loaded and anything touches the device
    std::vector<float> hgt;
    std::vector<unsigned char> hregion;
    int gt_w = 0, gt_rows = 0, nthr = 4;
    float thr[S2M2_EVAL_MAX_THR] = {0.5f, 1.f, 2.f, 4.f, 0.f, 0.f, 0.f, 0.f};
    if (gt_path) {
        const char* why = "";
        if (!read_pfm(gt_path, hgt, gt_w, gt_rows, why)) {
            fprintf(stderr, "s2m2_run_engine: --gt %s: %s\n", gt_path, why);
            return 1;
        }
        if (region_path) {
            hregion.resize(hgt.size());
            FILE* f = fopen(region_path, "rb");
            const bool ok = f && fread(hregion.data(), 1, hregion.size(), f) == hregion.size() && fgetc(f) == EOF;
            if (f) fclose(f);
            if (!ok) {
                fprintf(stderr, "s2m2_run_engine: --gt-region must be a raw uint8 file of the ground truth's %d x %d pixels\n", gt_w, gt_rows);
                return 1;
            }
        }
        if (thr_arg) {
            nthr = 0;
            for (const char* c = thr_arg; *c;) {
                char* end = nullptr;
                const float t = strtof(c, &end);
                if (end == c || nthr == S2M2_EVAL_MAX_THR || !(t > (nthr ? thr[nthr - 1] : 0.f)) || !isfinite(t) || (*end && *end != ','))
                    return fail("--thresholds: up to 8 numbers > 0, strictly increasing, separated by commas");
                thr[nthr++] = t;
                c = *end ? end + 1 : end;
            }
        }
        if (gt_min != gt_min) return fail("--gt-min: not a number");
    }
    if (s2m2_version() != S2M2_ABI_VERSION) return fail("libs2m2_hip.so was built from another ABI version than this program");

    s2m2_engine* eng = nullptr;
    if (s2m2_engine_load(pos[0], &eng) != 0) return fail_lib("cannot load the engine");
    s2m2_engine_info m;
    s2m2_engine_meta(eng, &m);
    if (m.image_dtype != S2M2_F32) return fail("this program feeds float32 images; the engine takes another image dtype");
    if (gt_path && (gt_rows % m.B != 0 || gt_rows / m.B > m.out_h || gt_w > m.out_w)) {
        fprintf(stderr, "s2m2_run_engine: --gt is %d x %d pixels; the engine needs B = %d stacked ground truths of at most %d x %d\n", gt_w, gt_rows,
                m.B, m.out_w, m.out_h);
        return 1;
    }
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
    // --min-size: the 3D outputs below read the map K22 leaves, with the filter already applied
    const float* disp3d = dout[0];
    int unfiltered3d = unfiltered;
    float* dseg = nullptr;
    if (min_size_arg) {
        Calib cal;
        if (!read_calib(calib_path, cal)) return fail("--calib: cannot read cam0 and baseline from the file");
        if (m.out_h != m.H || m.out_w != m.W) return fail("the 3D outputs need maps of the image's size (an engine without output_upsample)");
        const size_t npix = (size_t)m.H * m.W;
        const size_t ws_bytes = s2m2_segment_workspace_bytes(m.B, m.H, m.W);
        if (ws_bytes == 0) return fail("--min-size: extents too large");
        void* dws = nullptr;
        int32_t *dlabel = nullptr, *dstats = nullptr;
        unsigned char* dmask = nullptr;
        HIP_OK(hipMalloc(&dws, ws_bytes), "hipMalloc");
        HIP_OK(hipMalloc((void**)&dseg, map * sizeof(float)), "hipMalloc");
        HIP_OK(hipMalloc((void**)&dstats, m.B * 4 * sizeof(int32_t)), "hipMalloc");
        if (labels_path) HIP_OK(hipMalloc((void**)&dlabel, (size_t)m.B * npix * sizeof(int32_t)), "hipMalloc");
        if (segmask_path) HIP_OK(hipMalloc((void**)&dmask, (size_t)m.B * npix), "hipMalloc");
        s2m2_segment_desc sd;
        memset(&sd, 0, sizeof sd);
        s2m2_cloud_desc& cd = sd.cloud;
        cd.disp = dout[0]; cd.occ = dout[1]; cd.conf = dout[2];
        cd.image_dtype = S2M2_F32;
        cd.B = m.B; cd.H = m.H; cd.W = m.W; cd.Hp = m.out_h; cd.Wp = m.out_w;
        cd.unfiltered = unfiltered;
        cd.fx = cal.fx; cd.fy = cal.fy; cd.cx = cal.cx; cd.cy = cal.cy; cd.baseline = cal.baseline; cd.doffs = cal.doffs;
        cd.depth_scale = depth_scale; cd.depth_trunc = depth_trunc; cd.conf_min = conf_min; cd.occ_min = occ_min;
        sd.label = dlabel; sd.mask = dmask; sd.disp_out = dseg; sd.stats = dstats; sd.workspace = dws;
        sd.max_jump = max_jump; sd.min_size = min_size;
        if (s2m2_segment(&sd, s) != 0) return fail_lib("s2m2_segment failed");
        HIP_OK(hipStreamSynchronize(s), "s2m2_segment");
        std::vector<int32_t> hstats((size_t)m.B * 4);
        HIP_OK(hipMemcpy(hstats.data(), dstats, hstats.size() * sizeof(int32_t), hipMemcpyDeviceToHost), "download");
        if (labels_path) {
            std::vector<int32_t> hl32((size_t)m.B * npix);
            HIP_OK(hipMemcpy(hl32.data(), dlabel, hl32.size() * sizeof(int32_t), hipMemcpyDeviceToHost), "download");
            if (!write_bytes(labels_path, "", hl32.data(), hl32.size() * sizeof(int32_t))) return fail("cannot write the labels");
        }
        if (segmask_path) {
            std::vector<unsigned char> hm((size_t)m.B * npix);
            HIP_OK(hipMemcpy(hm.data(), dmask, hm.size(), hipMemcpyDeviceToHost), "download");
            if (!write_bytes(segmask_path, "", hm.data(), hm.size())) return fail("cannot write the segment mask");
        }
        if (repeat > 0) {
            hipEvent_t t0, t1;
            HIP_OK(hipEventCreate(&t0), "hipEventCreate");
            HIP_OK(hipEventCreate(&t1), "hipEventCreate");
            HIP_OK(hipEventRecord(t0, s), "hipEventRecord");
            for (int i = 0; i < repeat; ++i)
                if (s2m2_segment(&sd, s) != 0) return fail_lib("s2m2_segment failed");
            HIP_OK(hipEventRecord(t1, s), "hipEventRecord");
            HIP_OK(hipEventSynchronize(t1), "timed segment runs");
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, t0, t1), "hipEventElapsedTime");
            printf("{\"segment_kept\": %d, \"segment_components\": %d, \"segment_surviving\": %d, \"repeat\": %d, \"segment_us_per_pair\": %.2f}\n",
                   hstats[0], hstats[1], hstats[2], repeat, 1000.f * ms / repeat / m.B);
            (void)hipEventDestroy(t0);
            (void)hipEventDestroy(t1);
        }
        (void)hipFree(dws);
        (void)hipFree(dlabel);
        (void)hipFree(dmask);
        (void)hipFree(dstats);
        disp3d = dseg;
        unfiltered3d = 1;
    }
    if (calib_path && (ply_path || mesh_path)) {
        Calib cal;
        if (!read_calib(calib_path, cal)) return fail("--calib: cannot read cam0 and baseline from the file");
        if (m.out_h != m.H || m.out_w != m.W) return fail("the 3D outputs need maps of the image's size (an engine without output_upsample)");
        const size_t npix = (size_t)m.H * m.W;
        void *dimg = nullptr, *drec = nullptr, *dws = nullptr, *dfaces = nullptr;
        int32_t *dcount = nullptr, *dfcount = nullptr;
        const long long fcap = 2LL * (m.H - 1) * (m.W - 1);
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
        const size_t ws_bytes = mesh_path ? s2m2_mesh_workspace_bytes(m.B, m.H, m.W) : s2m2_cloud_workspace_bytes(m.B, m.H, m.W);
        if (ws_bytes == 0) return fail("the 3D outputs: extents too large");
        if (mesh_path) {
            HIP_OK(hipMalloc(&dfaces, (size_t)m.B * (fcap > 0 ? fcap : 1) * 12), "hipMalloc");
            HIP_OK(hipMalloc((void**)&dfcount, m.B * sizeof(int32_t)), "hipMalloc");
        }
        HIP_OK(hipMalloc(&drec, (size_t)m.B * npix * 16), "hipMalloc");
        HIP_OK(hipMalloc(&dws, ws_bytes), "hipMalloc");
        HIP_OK(hipMalloc((void**)&dcount, m.B * sizeof(int32_t)), "hipMalloc");
        if (depth_path) HIP_OK(hipMalloc((void**)&ddepth, (size_t)m.B * npix * sizeof(float)), "hipMalloc");
        s2m2_mesh_desc md;                                   // --mesh: one s2m2_mesh call writes the vertices (the --ply records) and the faces
        memset(&md, 0, sizeof md);
        s2m2_cloud_desc& cd = md.cloud;
        cd.disp = disp3d; cd.occ = dout[1]; cd.conf = dout[2];
        cd.image = image_path ? dimg : dl;
        cd.image_dtype = image_path ? 2 : S2M2_F32;
        cd.depth = ddepth; cd.records = drec; cd.count = dcount; cd.workspace = dws;
        cd.B = m.B; cd.H = m.H; cd.W = m.W; cd.Hp = m.out_h; cd.Wp = m.out_w;
        cd.unfiltered = unfiltered3d;
        cd.capacity = (long long)npix;
        cd.fx = cal.fx; cd.fy = cal.fy; cd.cx = cal.cx; cd.cy = cal.cy; cd.baseline = cal.baseline; cd.doffs = cal.doffs;
        cd.depth_scale = depth_scale; cd.depth_trunc = depth_trunc; cd.conf_min = conf_min; cd.occ_min = occ_min;
        md.faces = dfaces; md.face_count = dfcount; md.face_capacity = fcap; md.max_jump = max_jump;
        if (mesh_path) {
            if (s2m2_mesh(&md, s) != 0) return fail_lib("s2m2_mesh failed");
        } else if (s2m2_cloud(&cd, s) != 0) return fail_lib("s2m2_cloud failed");
        HIP_OK(hipStreamSynchronize(s), "s2m2_cloud");
        std::vector<int32_t> hcount(m.B), hfcount(m.B, 0);
        HIP_OK(hipMemcpy(hcount.data(), dcount, m.B * sizeof(int32_t), hipMemcpyDeviceToHost), "download");
        if (mesh_path) HIP_OK(hipMemcpy(hfcount.data(), dfcount, m.B * sizeof(int32_t), hipMemcpyDeviceToHost), "download");
        std::vector<unsigned char> hrec;
        std::vector<int32_t> hfaces;
        for (int b = 0; b < m.B; ++b) {
            hrec.resize((size_t)hcount[b] * 16);
            HIP_OK(hipMemcpy(hrec.data(), (const char*)drec + (size_t)b * npix * 16, hrec.size(), hipMemcpyDeviceToHost), "download");
            if (ply_path && !write_ply(pair_path(ply_path, m.B, b), hrec.data(), hcount[b])) return fail("cannot write the PLY file");
            if (mesh_path) {
                hfaces.resize((size_t)hfcount[b] * 3);
                HIP_OK(hipMemcpy(hfaces.data(), (const char*)dfaces + (size_t)b * fcap * 12, hfaces.size() * 4, hipMemcpyDeviceToHost), "download");
                if (!write_ply_mesh(pair_path(mesh_path, m.B, b), hrec.data(), hcount[b], hfaces.data(), hfcount[b]))
                    return fail("cannot write the mesh PLY file");
            }
        }
        if (depth_path) {
            std::vector<float> hd((size_t)m.B * npix);
            HIP_OK(hipMemcpy(hd.data(), ddepth, hd.size() * sizeof(float), hipMemcpyDeviceToHost), "download");
            if (!write_raw(depth_path, hd)) return fail("cannot write the depth map");
        }
        if (repeat > 0 && mesh_path) {
            hipEvent_t t0, t1;
            HIP_OK(hipEventCreate(&t0), "hipEventCreate");
            HIP_OK(hipEventCreate(&t1), "hipEventCreate");
            HIP_OK(hipEventRecord(t0, s), "hipEventRecord");
            for (int i = 0; i < repeat; ++i)
                if (s2m2_mesh(&md, s) != 0) return fail_lib("s2m2_mesh failed");
            HIP_OK(hipEventRecord(t1, s), "hipEventRecord");
            HIP_OK(hipEventSynchronize(t1), "timed mesh runs");
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, t0, t1), "hipEventElapsedTime");
            printf("{\"mesh_vertices\": %d, \"mesh_faces\": %d, \"repeat\": %d, \"mesh_us_per_pair\": %.2f}\n", hcount[0], hfcount[0], repeat,
                   1000.f * ms / repeat / m.B);
            (void)hipEventDestroy(t0);
            (void)hipEventDestroy(t1);
        }
        if (repeat > 0 && ply_path) {
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
        (void)hipFree(dfaces);
        (void)hipFree(dfcount);
    }
    if (register_cam) {
        Calib cal;
        if (!read_calib(calib_path, cal)) return fail("--calib: cannot read cam0 and baseline from the file");
        if (m.out_h != m.H || m.out_w != m.W) return fail("the 3D outputs need maps of the image's size (an engine without output_upsample)");
        TargetCamera cam;
        if (strcmp(register_cam, "right") == 0) {
            if (!cal.have_cam1) return fail("--register right: the calib file has no cam1");
            cam.width = m.W; cam.height = m.H;
            cam.fx = cal.cam1[0]; cam.fy = cal.cam1[1]; cam.cx = cal.cam1[2]; cam.cy = cal.cam1[3];
            cam.t[0] = -cal.baseline / depth_scale;
        } else if (!read_camera(register_cam, cam)) return fail("--register: the word right, or a file with width=, height= and cam=[fx 0 cx; 0 fy cy; 0 0 1]");
        const size_t ws_bytes = s2m2_register_workspace_bytes(m.B, cam.height, cam.width);
        if (ws_bytes == 0) return fail("--register: target extents too large");
        const size_t tpix = (size_t)cam.height * cam.width;
        void *dimg = nullptr, *dws = nullptr;
        float* dd = nullptr;
        int32_t *di = nullptr, *dcount = nullptr;
        unsigned char* dc = nullptr;
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
        HIP_OK(hipMalloc(&dws, ws_bytes), "hipMalloc");
        HIP_OK(hipMalloc((void**)&dd, (size_t)m.B * tpix * sizeof(float)), "hipMalloc");
        HIP_OK(hipMalloc((void**)&dcount, m.B * sizeof(int32_t)), "hipMalloc");
        if (reg_index_path) HIP_OK(hipMalloc((void**)&di, (size_t)m.B * tpix * sizeof(int32_t)), "hipMalloc");
        if (reg_image_path) HIP_OK(hipMalloc((void**)&dc, (size_t)m.B * 3 * tpix), "hipMalloc");
        s2m2_register_desc rd;
        memset(&rd, 0, sizeof rd);
        s2m2_cloud_desc& cd = rd.cloud;
        cd.disp = disp3d; cd.occ = dout[1]; cd.conf = dout[2];
        cd.image = image_path ? dimg : dl;
        cd.image_dtype = image_path ? 2 : S2M2_F32;
        cd.B = m.B; cd.H = m.H; cd.W = m.W; cd.Hp = m.out_h; cd.Wp = m.out_w;
        cd.unfiltered = unfiltered3d;
        cd.fx = cal.fx; cd.fy = cal.fy; cd.cx = cal.cx; cd.cy = cal.cy; cd.baseline = cal.baseline; cd.doffs = cal.doffs;
        cd.depth_scale = depth_scale; cd.depth_trunc = depth_trunc; cd.conf_min = conf_min; cd.occ_min = occ_min;
        rd.Ht = cam.height; rd.Wt = cam.width; rd.splat = splat;
        rd.fx_t = cam.fx; rd.fy_t = cam.fy; rd.cx_t = cam.cx; rd.cy_t = cam.cy;
        memcpy(rd.R, cam.R, sizeof rd.R);
        memcpy(rd.t, cam.t, sizeof rd.t);
        rd.depth_t = dd; rd.index_t = di; rd.image_t = dc; rd.count = dcount; rd.workspace = dws;
        if (s2m2_register(&rd, s) != 0) return fail_lib("s2m2_register failed");
        HIP_OK(hipStreamSynchronize(s), "s2m2_register");
        std::vector<int32_t> hcount(m.B);
        HIP_OK(hipMemcpy(hcount.data(), dcount, m.B * sizeof(int32_t), hipMemcpyDeviceToHost), "download");
        {
            std::vector<float> hd((size_t)m.B * tpix);
            HIP_OK(hipMemcpy(hd.data(), dd, hd.size() * sizeof(float), hipMemcpyDeviceToHost), "download");
            for (int b = 0; b < m.B; ++b)
                if (!write_bytes(pair_path(reg_depth_path, m.B, b, ".f32"), "", hd.data() + (size_t)b * tpix, tpix * sizeof(float)))
                    return fail("cannot write the registered depth map");
        }
        if (reg_index_path) {
            std::vector<int32_t> hidx((size_t)m.B * tpix);
            HIP_OK(hipMemcpy(hidx.data(), di, hidx.size() * sizeof(int32_t), hipMemcpyDeviceToHost), "download");
            for (int b = 0; b < m.B; ++b)
                if (!write_bytes(pair_path(reg_index_path, m.B, b, ".i32"), "", hidx.data() + (size_t)b * tpix, tpix * sizeof(int32_t)))
                    return fail("cannot write the registered index map");
        }
        if (reg_image_path) {
            std::vector<unsigned char> planar((size_t)m.B * 3 * tpix), rgb(3 * tpix);
            HIP_OK(hipMemcpy(planar.data(), dc, planar.size(), hipMemcpyDeviceToHost), "download");
            char head[64];
            snprintf(head, sizeof head, "P6\n%d %d\n255\n", cam.width, cam.height);
            for (int b = 0; b < m.B; ++b) {
                for (size_t i = 0; i < tpix; ++i)
                    for (int ch = 0; ch < 3; ++ch) rgb[3 * i + ch] = planar[((size_t)b * 3 + ch) * tpix + i];
                if (!write_bytes(pair_path(reg_image_path, m.B, b, ".ppm"), head, rgb.data(), rgb.size())) return fail("cannot write the registered image");
            }
        }
        if (repeat > 0) {
            hipEvent_t t0, t1;
            HIP_OK(hipEventCreate(&t0), "hipEventCreate");
            HIP_OK(hipEventCreate(&t1), "hipEventCreate");
            HIP_OK(hipEventRecord(t0, s), "hipEventRecord");
            for (int i = 0; i < repeat; ++i)
                if (s2m2_register(&rd, s) != 0) return fail_lib("s2m2_register failed");
            HIP_OK(hipEventRecord(t1, s), "hipEventRecord");
            HIP_OK(hipEventSynchronize(t1), "timed register runs");
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, t0, t1), "hipEventElapsedTime");
            printf("{\"register_covered\": %d, \"repeat\": %d, \"register_us_per_pair\": %.2f}\n", hcount[0], repeat, 1000.f * ms / repeat / m.B);
            (void)hipEventDestroy(t0);
            (void)hipEventDestroy(t1);
        }
        (void)hipFree(dimg);
        (void)hipFree(dws);
        (void)hipFree(dd);
        (void)hipFree(di);
        (void)hipFree(dc);
        (void)hipFree(dcount);
    }
    if (gt_path) {
        const int gt_h = gt_rows / m.B;
        float* dgt = nullptr;
        unsigned char* dregion = nullptr;
        void* dws = nullptr;
        unsigned long long* dstats = nullptr;
        const size_t ws_bytes = s2m2_eval_workspace_bytes(m.B, gt_h, gt_w), nwords = (size_t)m.B * S2M2_EVAL_WORDS;
        if (ws_bytes == 0) return fail("--gt: extents too large");
        HIP_OK(hipMalloc((void**)&dgt, hgt.size() * sizeof(float)), "hipMalloc");
        HIP_OK(hipMemcpy(dgt, hgt.data(), hgt.size() * sizeof(float), hipMemcpyHostToDevice), "upload");
        if (region_path) {
            HIP_OK(hipMalloc((void**)&dregion, hregion.size()), "hipMalloc");
            HIP_OK(hipMemcpy(dregion, hregion.data(), hregion.size(), hipMemcpyHostToDevice), "upload");
        }
        HIP_OK(hipMalloc(&dws, ws_bytes), "hipMalloc");
        HIP_OK(hipMalloc((void**)&dstats, nwords * sizeof(unsigned long long)), "hipMalloc");
        s2m2_eval_desc ed;
        memset(&ed, 0, sizeof ed);
        ed.disp = dout[0]; ed.occ = dout[1]; ed.conf = dout[2];
        ed.gt = dgt; ed.region = dregion; ed.workspace = dws; ed.stats = dstats;
        ed.B = m.B; ed.H = gt_h; ed.W = gt_w; ed.Hp = m.out_h; ed.Wp = m.out_w;
        ed.nthr = nthr;
        for (int t = 0; t < nthr; ++t) ed.thr[t] = thr[t];
        ed.d1_abs = 3.f; ed.d1_rel = 0.05f;
        ed.gt_min = (float)gt_min; ed.conf_min = (float)conf_min; ed.occ_min = (float)occ_min;
        if (s2m2_disp_eval(&ed, s) != 0) return fail_lib("s2m2_disp_eval failed");
        HIP_OK(hipStreamSynchronize(s), "s2m2_disp_eval");
        std::vector<unsigned long long> hs(nwords);
        HIP_OK(hipMemcpy(hs.data(), dstats, nwords * sizeof(unsigned long long), hipMemcpyDeviceToHost), "download");
        FILE* f = fopen(metrics_path, "w");
        if (!f) return fail("cannot write the metrics");
        fprintf(f, "{\"B\": %d, \"H\": %d, \"W\": %d, \"gt_min\": ", m.B, gt_h, gt_w);
        if (isfinite(gt_min)) fprintf(f, "%.9g", gt_min);
        else fprintf(f, "null");
        fprintf(f, ", \"conf_min\": %.9g, \"occ_min\": %.9g, \"thresholds\": [", conf_min, occ_min);
        for (int t = 0; t < nthr; ++t) fprintf(f, "%s%.9g", t ? ", " : "", (double)thr[t]);
        fprintf(f, "],\n \"pairs\": [");
        for (int b = 0; b < m.B; ++b) {
            const unsigned long long* w = hs.data() + (size_t)b * S2M2_EVAL_WORDS;
            fprintf(f, "%s\n  {", b ? "," : "");
            json_block(f, w + S2M2_EVAL_ALL, thr, nthr);
            fprintf(f, ", ");
            json_number(f, "a50", eval_quantile(w + S2M2_EVAL_HIST, 0.5), ", ");
            json_number(f, "a90", eval_quantile(w + S2M2_EVAL_HIST, 0.9), ", ");
            json_number(f, "a95", eval_quantile(w + S2M2_EVAL_HIST, 0.95), ", ");
            json_number(f, "a99", eval_quantile(w + S2M2_EVAL_HIST, 0.99), ", ");
            json_number(f, "density", (double)w[S2M2_EVAL_KEPT + S2M2_EVAL_N_EVAL] / (double)w[S2M2_EVAL_ALL + S2M2_EVAL_N_EVAL], ",\n   ");
            fprintf(f, "\"kept\": {");
            json_block(f, w + S2M2_EVAL_KEPT, thr, nthr);
            fprintf(f, "},\n   \"words\": [");
            for (int i = 0; i < S2M2_EVAL_WORDS; ++i) fprintf(f, "%s%llu", i ? ", " : "", w[i]);
            fprintf(f, "]}");
        }
        fprintf(f, "\n ]}\n");
        if (fclose(f) != 0) return fail("cannot write the metrics");
        if (repeat > 0) {
            hipEvent_t t0, t1;
            HIP_OK(hipEventCreate(&t0), "hipEventCreate");
            HIP_OK(hipEventCreate(&t1), "hipEventCreate");
            HIP_OK(hipEventRecord(t0, s), "hipEventRecord");
            for (int i = 0; i < repeat; ++i)
                if (s2m2_disp_eval(&ed, s) != 0) return fail_lib("s2m2_disp_eval failed");
            HIP_OK(hipEventRecord(t1, s), "hipEventRecord");
            HIP_OK(hipEventSynchronize(t1), "timed evaluation runs");
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, t0, t1), "hipEventElapsedTime");
            printf("{\"eval_pixels\": %llu, \"repeat\": %d, \"eval_us_per_pair\": %.2f}\n", hs[S2M2_EVAL_N_EVAL], repeat, 1000.f * ms / repeat / m.B);
            (void)hipEventDestroy(t0);
            (void)hipEventDestroy(t1);
        }
        (void)hipFree(dgt);
        (void)hipFree(dregion);
        (void)hipFree(dws);
        (void)hipFree(dstats);
    }
    s2m2_engine_destroy(eng);
    for (auto& p : dout) (void)hipFree(p);
    (void)hipFree(dseg);
    (void)hipFree(dl);
    (void)hipFree(dr);
    (void)hipStreamDestroy(s);
    return 0;
}
