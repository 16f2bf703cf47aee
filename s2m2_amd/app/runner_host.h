// The host side of s2m2_run_engine (run_engine.cpp): everything that needs no device -- the options, the readers of the files the program is
// given (calib, camera, PFM, raw), the names and writers of the files it leaves, the evaluation's derived numbers.  Plain C++ over the C header;
// nothing of HIP, so tools/runner_host_checks.cpp exercises all of it on a machine without a GPU.
#ifndef S2M2_RUNNER_HOST_H
#define S2M2_RUNNER_HOST_H

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "s2m2_hip.h"

inline const char* const USAGE =
    "usage: s2m2_run_engine ENGINE LEFT RIGHT [--out DIR] [--repeat N] [--calib FILE [--image LEFT.u8] [--depth-trunc M] [--depth-scale S] "
    "[--conf-min X] [--occ-min X] [--unfiltered] [--ply OUT.ply] [--mesh OUT.ply [--max-jump X]] [--depth OUT.f32] "
    "[--register CAM [--splat N] --register-depth OUT.f32 [--register-image OUT.ppm] [--register-index OUT.i32]] "
    "[--min-size N [--labels OUT.i32] [--segment-mask OUT.u8]] [--voxel SIZE --voxel-ply OUT.ply [--voxel-max N]] "
    "[--normals OUT.f32 [--normals-image OUT.ppm] [--normals-radius R] [--normals-min-cos X]] "
    "[--smooth R --smooth-sigma-r X --smooth-max-jump X [--smooth-sigma-s X] [--smooth-out OUT.f32]]] [--gt FILE.pfm [--gt-region FILE.u8] [--gt-min X] "
    "[--thresholds a,b,c] --metrics OUT.json]"
    " | s2m2_run_engine ENGINE --tsdf-frames LIST.txt --tsdf-dims NX,NY,NZ --tsdf-voxel VS --tsdf-origin X,Y,Z [--tsdf-trunc T] "
    "[--tsdf-min-weight N] [--tsdf-carve] --calib FILE --tsdf-ply OUT.ply [--tsdf-mesh OUT.ply] [--tsdf-render POSE [--tsdf-render-depth OUT.f32] "
    "[--tsdf-render-image OUT.u8] [--tsdf-render-step X] [--tsdf-render-min-weight N]] [--tsdf-track [--tsdf-track-iters N] [--tsdf-track-dist D] "
    "[--tsdf-poses-out FILE]] [--smooth R --smooth-sigma-r X --smooth-max-jump X [--smooth-sigma-s X]] [--depth-trunc M] [--depth-scale S] [--conf-min X] [--occ-min X] "
    "[--unfiltered]";

// ---- options: every option as it stands on the command line (null: not given), then the numbers check_options parses from them
struct Options {
    const char* pos[3] = {nullptr, nullptr, nullptr};    // ENGINE LEFT RIGHT
    int npos = 0;
    const char *out_dir = nullptr, *repeat_arg = nullptr;
    const char *calib_path = nullptr, *image_path = nullptr, *ply_path = nullptr, *depth_path = nullptr, *mesh_path = nullptr;
    const char *depth_trunc_arg = nullptr, *depth_scale_arg = nullptr, *conf_min_arg = nullptr, *occ_min_arg = nullptr, *unfiltered_arg = nullptr;
    const char* max_jump_arg = nullptr;
    const char *register_cam = nullptr, *reg_depth_path = nullptr, *reg_image_path = nullptr, *reg_index_path = nullptr, *splat_arg = nullptr;
    const char *min_size_arg = nullptr, *labels_path = nullptr, *segmask_path = nullptr;
    const char *voxel_arg = nullptr, *voxel_ply_path = nullptr, *voxel_max_arg = nullptr;
    const char *normals_path = nullptr, *normals_image_path = nullptr, *normals_radius_arg = nullptr, *normals_min_cos_arg = nullptr;
    const char *smooth_arg = nullptr, *smooth_sigma_r_arg = nullptr, *smooth_max_jump_arg = nullptr, *smooth_sigma_s_arg = nullptr;
    const char* smooth_out_path = nullptr;
    const char *gt_path = nullptr, *region_path = nullptr, *metrics_path = nullptr, *thr_arg = nullptr, *gt_min_arg = nullptr;
    const char *tsdf_frames_path = nullptr, *tsdf_dims_arg = nullptr, *tsdf_voxel_arg = nullptr, *tsdf_origin_arg = nullptr;
    const char *tsdf_trunc_arg = nullptr, *tsdf_min_weight_arg = nullptr, *tsdf_carve_arg = nullptr, *tsdf_ply_path = nullptr;
    const char* tsdf_mesh_path = nullptr;
    const char *tsdf_render_arg = nullptr, *tsdf_render_depth_path = nullptr, *tsdf_render_image_path = nullptr;
    const char *tsdf_render_step_arg = nullptr, *tsdf_render_min_weight_arg = nullptr;
    const char *tsdf_track_arg = nullptr, *tsdf_track_iters_arg = nullptr, *tsdf_track_dist_arg = nullptr, *tsdf_poses_out_path = nullptr;

    int tsdf_dims[3] = {0, 0, 0}, tsdf_min_weight = 1, tsdf_carve = 0;
    double tsdf_voxel = 0.0, tsdf_trunc = 0.0, tsdf_origin[3] = {0, 0, 0};      // tsdf_trunc: 4 * tsdf_voxel unless --tsdf-trunc
    float tsdf_render_pose[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};          // --tsdf-render: [R | t] row-major, world -> camera
    double tsdf_render_step = 0.0;                       // tsdf_trunc / 2 unless --tsdf-render-step
    int tsdf_render_min_weight = 1;                      // tsdf_min_weight unless --tsdf-render-min-weight
    int tsdf_track = 0, tsdf_track_iters = 10;           // --tsdf-track (K27): the poses of the lines behind the first are tracked
    double tsdf_track_dist = 0.0;                        // tsdf_trunc unless --tsdf-track-dist
    int repeat = 0, splat = 2, unfiltered = 0;
    long long min_size = 1, voxel_max = 0;               // voxel_max 0: a quarter of the image's pixels
    double max_jump = 1.0, voxel_size = 0.0;
    int normals_radius = 1;                              // --normals (K28): the distance of the neighbours and the view gate
    double normals_min_cos = 0.0;
    int smooth_radius = 0;                               // --smooth (K29): the window, the two widths (sigma_s: radius / 2 unless given), the gate
    double smooth_sigma_s = 0.0, smooth_sigma_r = 0.0, smooth_max_jump = 0.0;
    double depth_trunc = 0.0, depth_scale = 1000.0, conf_min = 0.1, occ_min = 0.5, gt_min = 0.0;
};

// one row per option; a new option is one row here, one member above and, where it has rules, one line in check_options
struct OptionRow {
    const char* name;
    bool takes_value;                 // false: a flag, stored as its own name
    const char* Options::*dst;
};

inline const OptionRow OPTION_TABLE[] = {
    {"--out", true, &Options::out_dir},
    {"--repeat", true, &Options::repeat_arg},
    {"--calib", true, &Options::calib_path},
    {"--image", true, &Options::image_path},
    {"--ply", true, &Options::ply_path},
    {"--mesh", true, &Options::mesh_path},
    {"--max-jump", true, &Options::max_jump_arg},
    {"--depth", true, &Options::depth_path},
    {"--register", true, &Options::register_cam},
    {"--splat", true, &Options::splat_arg},
    {"--register-depth", true, &Options::reg_depth_path},
    {"--register-image", true, &Options::reg_image_path},
    {"--register-index", true, &Options::reg_index_path},
    {"--min-size", true, &Options::min_size_arg},
    {"--labels", true, &Options::labels_path},
    {"--segment-mask", true, &Options::segmask_path},
    {"--voxel", true, &Options::voxel_arg},
    {"--voxel-ply", true, &Options::voxel_ply_path},
    {"--voxel-max", true, &Options::voxel_max_arg},
    {"--normals", true, &Options::normals_path},
    {"--normals-image", true, &Options::normals_image_path},
    {"--normals-radius", true, &Options::normals_radius_arg},
    {"--normals-min-cos", true, &Options::normals_min_cos_arg},
    {"--smooth", true, &Options::smooth_arg},
    {"--smooth-sigma-r", true, &Options::smooth_sigma_r_arg},
    {"--smooth-max-jump", true, &Options::smooth_max_jump_arg},
    {"--smooth-sigma-s", true, &Options::smooth_sigma_s_arg},
    {"--smooth-out", true, &Options::smooth_out_path},
    {"--depth-trunc", true, &Options::depth_trunc_arg},
    {"--depth-scale", true, &Options::depth_scale_arg},
    {"--conf-min", true, &Options::conf_min_arg},
    {"--occ-min", true, &Options::occ_min_arg},
    {"--unfiltered", false, &Options::unfiltered_arg},
    {"--gt", true, &Options::gt_path},
    {"--gt-region", true, &Options::region_path},
    {"--gt-min", true, &Options::gt_min_arg},
    {"--thresholds", true, &Options::thr_arg},
    {"--metrics", true, &Options::metrics_path},
    {"--tsdf-frames", true, &Options::tsdf_frames_path},
    {"--tsdf-dims", true, &Options::tsdf_dims_arg},
    {"--tsdf-voxel", true, &Options::tsdf_voxel_arg},
    {"--tsdf-origin", true, &Options::tsdf_origin_arg},
    {"--tsdf-trunc", true, &Options::tsdf_trunc_arg},
    {"--tsdf-min-weight", true, &Options::tsdf_min_weight_arg},
    {"--tsdf-carve", false, &Options::tsdf_carve_arg},
    {"--tsdf-ply", true, &Options::tsdf_ply_path},
    {"--tsdf-mesh", true, &Options::tsdf_mesh_path},
    {"--tsdf-render", true, &Options::tsdf_render_arg},
    {"--tsdf-render-depth", true, &Options::tsdf_render_depth_path},
    {"--tsdf-render-image", true, &Options::tsdf_render_image_path},
    {"--tsdf-render-step", true, &Options::tsdf_render_step_arg},
    {"--tsdf-render-min-weight", true, &Options::tsdf_render_min_weight_arg},
    {"--tsdf-track", false, &Options::tsdf_track_arg},
    {"--tsdf-track-iters", true, &Options::tsdf_track_iters_arg},
    {"--tsdf-track-dist", true, &Options::tsdf_track_dist_arg},
    {"--tsdf-poses-out", true, &Options::tsdf_poses_out_path},
};

// "a,b,c": exactly three numbers, nothing behind them
inline bool parse_triple(const char* arg, double* v) {
    for (int i = 0; i < 3; ++i) {
        char* end = nullptr;
        v[i] = strtod(arg, &end);
        if (end == arg || *end != (i < 2 ? ',' : '\0')) return false;
        arg = end + 1;
    }
    return true;
}

// a finite number > 0, nothing behind it
inline bool parse_positive(const char* arg, double& v) {
    char* end = nullptr;
    v = strtod(arg, &end);
    return end != arg && !*end && v > 0.0 && isfinite(v);
}

// "a,b,...": exactly twelve finite numbers that fit a float, nothing behind them
inline bool parse_pose(const char* arg, float* v) {
    for (int i = 0; i < 12; ++i) {
        char* end = nullptr;
        v[i] = strtof(arg, &end);
        if (end == arg || *end != (i < 11 ? ',' : '\0') || !isfinite(v[i])) return false;
        arg = end + 1;
    }
    return true;
}

// the rules of the --smooth* options (K29), which both modes take; null: complete
inline const char* check_smooth_options(Options& o) {
    if (!o.smooth_arg) {
        if (o.smooth_sigma_r_arg || o.smooth_max_jump_arg || o.smooth_sigma_s_arg || o.smooth_out_path)
            return "--smooth-sigma-r, --smooth-max-jump, --smooth-sigma-s and --smooth-out need --smooth";
        return nullptr;
    }
    if (!o.smooth_sigma_r_arg || !o.smooth_max_jump_arg)
        return "--smooth needs --smooth-sigma-r and --smooth-max-jump: they depend on the rig's disparity noise and have no default";
    if (!o.calib_path) return "--smooth needs --calib";
    char* end = nullptr;
    const long long n = strtoll(o.smooth_arg, &end, 10);
    if (end == o.smooth_arg || *end || n < 1 || n > 8) return "--smooth: the radius, an integer in 1..8";
    o.smooth_radius = (int)n;
    o.smooth_sigma_s = 0.5 * (double)n;
    if (!parse_positive(o.smooth_sigma_r_arg, o.smooth_sigma_r)) return "--smooth-sigma-r: a finite number > 0";
    if (o.smooth_sigma_s_arg && !parse_positive(o.smooth_sigma_s_arg, o.smooth_sigma_s)) return "--smooth-sigma-s: a finite number > 0";
    o.smooth_max_jump = strtod(o.smooth_max_jump_arg, &end);
    if (end == o.smooth_max_jump_arg || *end || !(o.smooth_max_jump >= 0.0)) return "--smooth-max-jump: a number >= 0 (inf is allowed)";
    return nullptr;
}

// the rules of the --tsdf-* options (K24); null: complete.  The mode takes ENGINE alone: its pairs come from LIST
inline const char* check_tsdf_options(Options& o) {
    if (!o.tsdf_frames_path) return "the --tsdf-* options need --tsdf-frames";
    if (o.npos != 1) return "--tsdf-frames takes ENGINE alone: the pairs are named in LIST";
    if (!o.tsdf_dims_arg || !o.tsdf_voxel_arg || !o.tsdf_origin_arg || !o.tsdf_ply_path || !o.calib_path)
        return "--tsdf-frames needs --tsdf-dims, --tsdf-voxel, --tsdf-origin, --calib and --tsdf-ply";
    if (o.out_dir || o.repeat_arg || o.image_path || o.ply_path || o.mesh_path || o.depth_path || o.register_cam || o.min_size_arg || o.voxel_arg ||
        o.gt_path || o.max_jump_arg || o.normals_path || o.normals_image_path || o.normals_radius_arg || o.normals_min_cos_arg || o.smooth_out_path)
        return "--tsdf-frames comes without the options of a single pair";
    double d[3];
    if (!parse_triple(o.tsdf_dims_arg, d)) return "--tsdf-dims: three integers >= 1, NX,NY,NZ with NX*NY*NZ < 2^29";
    for (int i = 0; i < 3; ++i) {
        if (!(d[i] >= 1.0 && d[i] < 536870912.0 && d[i] == floor(d[i]))) return "--tsdf-dims: three integers >= 1, NX,NY,NZ with NX*NY*NZ < 2^29";
        o.tsdf_dims[i] = (int)d[i];
    }
    if (d[0] * d[1] * d[2] >= 536870912.0) return "--tsdf-dims: three integers >= 1, NX,NY,NZ with NX*NY*NZ < 2^29";
    if (!parse_positive(o.tsdf_voxel_arg, o.tsdf_voxel)) return "--tsdf-voxel: a number > 0";
    if (!parse_triple(o.tsdf_origin_arg, o.tsdf_origin) || !isfinite(o.tsdf_origin[0]) || !isfinite(o.tsdf_origin[1]) || !isfinite(o.tsdf_origin[2]))
        return "--tsdf-origin: three finite numbers X,Y,Z";
    o.tsdf_trunc = 4.0 * o.tsdf_voxel;
    if (o.tsdf_trunc_arg && !parse_positive(o.tsdf_trunc_arg, o.tsdf_trunc)) return "--tsdf-trunc: a number > 0";
    if (o.tsdf_min_weight_arg) {
        char* end = nullptr;
        const long long n = strtoll(o.tsdf_min_weight_arg, &end, 10);
        if (end == o.tsdf_min_weight_arg || *end || n < 1 || n > 32767) return "--tsdf-min-weight: an integer in 1..32767";
        o.tsdf_min_weight = (int)n;
    }
    o.tsdf_carve = o.tsdf_carve_arg != nullptr;
    // K25's size limit: an int32 face count, at most 5 faces per cell
    if (o.tsdf_mesh_path && d[0] * d[1] * d[2] > 429496729.0) return "--tsdf-mesh: NX*NY*NZ <= 429496729 (an int32 face count)";
    // --tsdf-render (K26): the pose, at least one of the two maps, the step and the weight a voxel needs
    if (!o.tsdf_render_arg && (o.tsdf_render_depth_path || o.tsdf_render_image_path || o.tsdf_render_step_arg || o.tsdf_render_min_weight_arg))
        return "the --tsdf-render-* options need --tsdf-render";
    o.tsdf_render_step = 0.5 * o.tsdf_trunc;
    o.tsdf_render_min_weight = o.tsdf_min_weight;
    if (o.tsdf_render_arg) {
        if (!o.tsdf_render_depth_path && !o.tsdf_render_image_path) return "--tsdf-render needs --tsdf-render-depth or --tsdf-render-image";
        if (!parse_pose(o.tsdf_render_arg, o.tsdf_render_pose)) return "--tsdf-render: twelve finite numbers, [R | t] row-major, separated by commas";
        if (o.tsdf_render_step_arg && !parse_positive(o.tsdf_render_step_arg, o.tsdf_render_step)) return "--tsdf-render-step: a number > 0";
        if (o.tsdf_render_min_weight_arg) {
            char* end = nullptr;
            const long long n = strtoll(o.tsdf_render_min_weight_arg, &end, 10);
            if (end == o.tsdf_render_min_weight_arg || *end || n < 1 || n > 32767) return "--tsdf-render-min-weight: an integer in 1..32767";
            o.tsdf_render_min_weight = (int)n;
        }
    }
    // --tsdf-track (K27): the iterations per frame and the correspondence gate
    if (!o.tsdf_track_arg && (o.tsdf_track_iters_arg || o.tsdf_track_dist_arg || o.tsdf_poses_out_path))
        return "--tsdf-track-iters, --tsdf-track-dist and --tsdf-poses-out need --tsdf-track";
    o.tsdf_track = o.tsdf_track_arg != nullptr;
    o.tsdf_track_dist = o.tsdf_trunc;
    if (o.tsdf_track_iters_arg) {
        char* end = nullptr;
        const long long n = strtoll(o.tsdf_track_iters_arg, &end, 10);
        if (end == o.tsdf_track_iters_arg || *end || n < 1 || n > 64) return "--tsdf-track-iters: an integer in 1..64";
        o.tsdf_track_iters = (int)n;
    }
    if (o.tsdf_track_dist_arg && !parse_positive(o.tsdf_track_dist_arg, o.tsdf_track_dist)) return "--tsdf-track-dist: a number > 0";
    return nullptr;
}

// false: an unknown option, an option without its value or a fourth positional (the caller prints USAGE); a repeated option: the last one
inline bool parse_options(int argc, char** argv, Options& o) {
    for (int i = 1; i < argc; ++i) {
        const OptionRow* row = nullptr;
        for (const OptionRow& r : OPTION_TABLE)
            if (strcmp(argv[i], r.name) == 0) row = &r;
        if (row && !row->takes_value) o.*row->dst = argv[i];
        else if (row && i + 1 < argc) o.*row->dst = argv[++i];
        else if (o.npos < 3 && argv[i][0] != '-') o.pos[o.npos++] = argv[i];
        else return false;
    }
    return true;
}

// the numbers of the options and the rules between options, in the order the messages have always come in; null: the options are complete
inline const char* check_options(Options& o) {
    if (o.repeat_arg) o.repeat = atoi(o.repeat_arg);
    if (o.depth_trunc_arg) o.depth_trunc = atof(o.depth_trunc_arg);
    if (o.depth_scale_arg) o.depth_scale = atof(o.depth_scale_arg);
    if (o.conf_min_arg) o.conf_min = atof(o.conf_min_arg);
    if (o.occ_min_arg) o.occ_min = atof(o.occ_min_arg);
    if (o.gt_min_arg) o.gt_min = atof(o.gt_min_arg);
    o.unfiltered = o.unfiltered_arg != nullptr;
    if (const char* msg = check_smooth_options(o)) return msg;
    if (o.tsdf_frames_path || o.tsdf_dims_arg || o.tsdf_voxel_arg || o.tsdf_origin_arg || o.tsdf_trunc_arg || o.tsdf_min_weight_arg || o.tsdf_carve_arg ||
        o.tsdf_ply_path || o.tsdf_mesh_path || o.tsdf_render_arg || o.tsdf_render_depth_path || o.tsdf_render_image_path || o.tsdf_render_step_arg ||
        o.tsdf_render_min_weight_arg || o.tsdf_track_arg || o.tsdf_track_iters_arg || o.tsdf_track_dist_arg || o.tsdf_poses_out_path)
        return check_tsdf_options(o);
    if (o.npos != 3 || o.repeat < 0) return USAGE;
    if (o.mesh_path && !o.calib_path) return "--calib and --mesh come together";
    if (o.register_cam && (!o.calib_path || !o.reg_depth_path)) return "--register needs --calib and --register-depth";
    if (!o.register_cam && (o.reg_depth_path || o.reg_image_path || o.reg_index_path || o.splat_arg)) return "--splat and --register-* need --register";
    if (o.splat_arg) {
        o.splat = atoi(o.splat_arg);
        if (o.splat < 1 || o.splat > 4) return "--splat: 1, 2, 3 or 4";
    }
    if (o.min_size_arg && !o.calib_path) return "--min-size needs --calib";
    if (!o.min_size_arg && (o.labels_path || o.segmask_path)) return "--labels and --segment-mask need --min-size";
    if (o.min_size_arg) {
        char* end = nullptr;
        o.min_size = strtoll(o.min_size_arg, &end, 10);
        if (end == o.min_size_arg || *end || o.min_size < 1 || o.min_size > (1LL << 30)) return "--min-size: an integer >= 1 (at most 2^30)";
    }
    if ((o.voxel_arg == nullptr) != (o.voxel_ply_path == nullptr)) return "--voxel and --voxel-ply come together";
    if (o.voxel_max_arg && !o.voxel_arg) return "--voxel-max needs --voxel";
    if (o.voxel_arg && !o.calib_path) return "--voxel needs --calib";
    if (o.voxel_arg) {
        char* end = nullptr;
        o.voxel_size = strtod(o.voxel_arg, &end);
        if (end == o.voxel_arg || *end || !(o.voxel_size > 0.0) || !isfinite(o.voxel_size)) return "--voxel: a number > 0";
    }
    if (o.voxel_max_arg) {
        char* end = nullptr;
        o.voxel_max = strtoll(o.voxel_max_arg, &end, 10);
        if (end == o.voxel_max_arg || *end || o.voxel_max < 1 || o.voxel_max > (1LL << 29)) return "--voxel-max: an integer >= 1 (at most 2^29)";
    }
    if (o.normals_path && !o.calib_path) return "--normals needs --calib";
    if (!o.normals_path && (o.normals_image_path || o.normals_radius_arg || o.normals_min_cos_arg))
        return "--normals-image, --normals-radius and --normals-min-cos need --normals";
    if (o.normals_radius_arg) {
        char* end = nullptr;
        const long long n = strtoll(o.normals_radius_arg, &end, 10);
        if (end == o.normals_radius_arg || *end || n < 1 || n > 8) return "--normals-radius: an integer in 1..8";
        o.normals_radius = (int)n;
    }
    if (o.normals_min_cos_arg) {
        char* end = nullptr;
        o.normals_min_cos = strtod(o.normals_min_cos_arg, &end);
        if (end == o.normals_min_cos_arg || *end || !isfinite(o.normals_min_cos) || !(o.normals_min_cos < 1.0)) return "--normals-min-cos: a finite number < 1";
    }
    if (!o.mesh_path && !o.register_cam && !o.min_size_arg && !o.voxel_arg && !o.normals_path && !o.smooth_arg &&
        (o.calib_path == nullptr) != (o.ply_path == nullptr))
        return "--calib and --ply come together";
    if ((o.register_cam || o.min_size_arg || o.voxel_arg || o.normals_path || o.smooth_arg) && !o.mesh_path && !o.ply_path && o.depth_path) return "--depth needs --ply or --mesh";
    if (o.max_jump_arg && !o.mesh_path && !o.min_size_arg && !o.normals_path) return "--max-jump needs --mesh or --min-size";
    if (o.max_jump_arg) {
        char* end = nullptr;
        o.max_jump = strtod(o.max_jump_arg, &end);
        if (end == o.max_jump_arg || *end || !(o.max_jump >= 0.0)) return "--max-jump: a number >= 0 (inf is allowed)";
    }
    if (!o.calib_path && (o.image_path || o.depth_path)) return "--image and --depth need --calib and --ply";
    if ((o.gt_path == nullptr) != (o.metrics_path == nullptr)) return "--gt and --metrics come together";
    if (!o.gt_path && (o.region_path || o.thr_arg)) return "--gt-region and --thresholds need --gt and --metrics";
    return nullptr;
}

// ---- readers
// a file of exactly `bytes` bytes
inline bool read_exact(const char* path, void* data, size_t bytes) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t n = fread(data, 1, bytes, f);
    const bool at_end = fgetc(f) == EOF;
    fclose(f);
    return n == bytes && at_end;
}

// a raw little-endian float32 file of exactly v.size() values
inline bool read_raw(const char* path, std::vector<float>& v) { return read_exact(path, v.data(), v.size() * sizeof(float)); }

// a raw uint8 file of exactly v.size() bytes (--image, --gt-region)
inline bool read_raw_u8(const char* path, std::vector<unsigned char>& v) { return read_exact(path, v.data(), v.size()); }

// cam0=[fx 0 cx; 0 fy cy; 0 0 1], doffs=, baseline= of a Middlebury calib.txt; every other key is ignored
struct Calib {
    double fx = 0, fy = 0, cx = 0, cy = 0, doffs = 0, baseline = 0;
    double cam1[4] = {0, 0, 0, 0};      // fx, fy, cx, cy of cam1 (--register right)
    bool have_cam0 = false, have_baseline = false, have_cam1 = false;
};

inline bool read_calib(const char* path, Calib& c) {
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

// the target camera of --register: a text file in the calib file's syntax (see the head of run_engine.cpp)
struct TargetCamera {
    int width = 0, height = 0;
    double fx = 0, fy = 0, cx = 0, cy = 0;
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double t[3] = {0, 0, 0};
};

inline bool read_camera(const char* path, TargetCamera& c) {
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

// --tsdf-frames LIST: one frame per line -- LEFT.f32 RIGHT.f32 IMAGE.u8 and the twelve numbers of [R | t] row-major (world -> camera, t in the
// unit of z); empty lines and lines that start with # are skipped.  The file names are used as they stand and hold no blanks.  With `track`
// (--tsdf-track) the twelve numbers are optional behind the first frame -- they are ignored there --, all twelve or none
struct TsdfFrame {
    std::string left, right, image;
    float pose[12];
};

// "": fine, else the message (with the line's number)
inline std::string read_tsdf_frames(const char* path, std::vector<TsdfFrame>& frames, bool track = false) {
    FILE* f = fopen(path, "r");
    if (!f) return std::string("--tsdf-frames ") + path + ": cannot open the file";
    char line[4096];
    std::string msg;
    for (int no = 1; msg.empty() && fgets(line, sizeof line, f); ++no) {
        const char* c = line + strspn(line, " \t\r\n");
        if (!*c || *c == '#') continue;
        char name[3][1024];
        int used = 0;
        TsdfFrame fr;
        bool ok = sscanf(c, "%1023s %1023s %1023s%n", name[0], name[1], name[2], &used) == 3;
        c += used;
        const bool bare = ok && track && !frames.empty() && !c[strspn(c, " \t\r\n")];      // a tracked frame without a pose
        for (int i = 0; i < 12; ++i) fr.pose[i] = 0.f;
        for (int i = 0; ok && !bare && i < 12; ++i) {
            char* end = nullptr;
            fr.pose[i] = strtof(c, &end);
            ok = end != c && isfinite(fr.pose[i]);
            c = end;
        }
        ok = ok && !c[strspn(c, " \t\r\n")];
        if (!ok) msg = std::string("--tsdf-frames ") + path + ": line " + std::to_string(no) + ": LEFT.f32 RIGHT.f32 IMAGE.u8 and twelve finite pose numbers";
        if (ok) {
            fr.left = name[0]; fr.right = name[1]; fr.image = name[2];
            frames.push_back(fr);
        }
    }
    fclose(f);
    if (msg.empty() && frames.empty()) msg = std::string("--tsdf-frames ") + path + ": no frame";
    return msg;
}

// the largest distance from the centre of the camera `pose` ([R | t] row-major, world -> camera: the centre is -R^T t) to a corner of the grid:
// no surface of the volume lies deeper along any ray (--tsdf-render's z_far)
inline double tsdf_far_corner(const float* pose, const int* dims, const double* origin, double voxel) {
    double centre[3], far = 0.0;
    for (int a = 0; a < 3; ++a) centre[a] = -((double)pose[a] * pose[3] + (double)pose[4 + a] * pose[7] + (double)pose[8 + a] * pose[11]);
    for (int c = 0; c < 8; ++c) {
        double d2 = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double x = origin[a] + ((c >> a) & 1) * (dims[a] - 1) * voxel - centre[a];
            d2 += x * x;
        }
        far = fmax(far, sqrt(d2));
    }
    return far;
}

// greyscale PFM: "Pf", "width height", "scale" (negative: little-endian), then the rows bottom to top -> rows top to bottom
inline bool read_pfm(const char* path, std::vector<float>& v, int& width, int& height, const char*& why) {
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

// --thresholds a,b,c: up to S2M2_EVAL_MAX_THR finite numbers > 0, strictly increasing (a trailing comma passes; "": no threshold)
inline bool parse_thresholds(const char* arg, float* thr, int& nthr) {
    nthr = 0;
    for (const char* c = arg; *c;) {
        char* end = nullptr;
        const float t = strtof(c, &end);
        if (end == c || nthr == S2M2_EVAL_MAX_THR || !(t > (nthr ? thr[nthr - 1] : 0.f)) || !isfinite(t) || (*end && *end != ',')) return false;
        thr[nthr++] = t;
        c = *end ? end + 1 : end;
    }
    return true;
}

// what --gt, --gt-region, --thresholds and --gt-min give the evaluation stage
struct GroundTruth {
    std::vector<float> gt;                   // w x rows: the B ground truths stacked
    std::vector<unsigned char> region;
    int w = 0, rows = 0, nthr = 4;
    float thr[S2M2_EVAL_MAX_THR] = {0.5f, 1.f, 2.f, 4.f, 0.f, 0.f, 0.f, 0.f};
};

// parsed and validated before the engine is loaded and anything touches the device; "": fine (also without --gt), else the message
inline std::string read_ground_truth(const Options& o, GroundTruth& g) {
    if (!o.gt_path) return "";
    const char* why = "";
    if (!read_pfm(o.gt_path, g.gt, g.w, g.rows, why)) return std::string("--gt ") + o.gt_path + ": " + why;
    if (o.region_path) {
        g.region.resize(g.gt.size());
        if (!read_raw_u8(o.region_path, g.region))
            return "--gt-region must be a raw uint8 file of the ground truth's " + std::to_string(g.w) + " x " + std::to_string(g.rows) + " pixels";
    }
    if (o.thr_arg && !parse_thresholds(o.thr_arg, g.thr, g.nthr)) return "--thresholds: up to 8 numbers > 0, strictly increasing, separated by commas";
    if (o.gt_min != o.gt_min) return "--gt-min: not a number";
    return "";
}

// ---- the input half of s2m2_cloud_desc, shared by K15 / K20, K21 and K22: maps, image, extents, camera and filter numbers.  `unfiltered` is
// the option's, or 1 behind K22 (the filter is in the map then)
inline void fill_cloud_inputs(s2m2_cloud_desc& cd, const s2m2_engine_info& m, const float* disp, const float* occ, const float* conf,
                              const void* image, int image_dtype, int unfiltered, const Calib& cal, const Options& o) {
    cd.disp = disp; cd.occ = occ; cd.conf = conf;
    cd.image = image;
    cd.image_dtype = image_dtype;
    cd.B = m.B; cd.H = m.H; cd.W = m.W; cd.Hp = m.out_h; cd.Wp = m.out_w;
    cd.unfiltered = unfiltered;
    cd.fx = cal.fx; cd.fy = cal.fy; cd.cx = cal.cx; cd.cy = cal.cy; cd.baseline = cal.baseline; cd.doffs = cal.doffs;
    cd.depth_scale = o.depth_scale; cd.depth_trunc = o.depth_trunc; cd.conf_min = o.conf_min; cd.occ_min = o.occ_min;
}

// ---- writers
// OUT.ply, or OUT.<b>.ply for engines of more than one pair (a trailing ".ply" of OUT is dropped first); --register-image: ".ppm"
inline std::string pair_path(const char* out, int B, int b, const char* ext = ".ply") {
    std::string stem = out;
    if (B <= 1) return stem;
    const size_t ne = strlen(ext);
    if (stem.size() > ne && stem.compare(stem.size() - ne, ne, ext) == 0) stem.resize(stem.size() - ne);
    return stem + "." + std::to_string(b) + ext;
}

inline bool write_bytes(const std::string& path, const char* head, const void* data, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(head, 1, strlen(head), f) == strlen(head) && fwrite(data, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

inline bool write_ply(const std::string& path, const void* records, long long n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %lld\nproperty float x\nproperty float y\nproperty float z\n"
               "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n", n);
    const bool ok = fwrite(records, 16, (size_t)n, f) == (size_t)n;
    return fclose(f) == 0 && ok;
}

// the same vertices, then every face as a count byte (3) and three little-endian int32 vertex indices: 13 bytes
inline bool write_ply_mesh(const std::string& path, const void* records, long long n, const int32_t* faces, long long nf) {
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

inline void json_number(FILE* f, const char* key, double x, const char* tail) {
    if (isfinite(x)) fprintf(f, "\"%s\": %.17g%s", key, x, tail);
    else fprintf(f, "\"%s\": null%s", key, tail);
}

// the derived numbers of one ALL / KEPT block (s2m2_amd/evaluate.py: EvalStats, the same arithmetic in double)
inline void json_block(FILE* f, const unsigned long long* blk, const float* thr, int nthr) {
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
inline double eval_quantile(const unsigned long long* hist, double p) {
    unsigned long long n = 0, cum = 0;
    for (int i = 0; i < S2M2_EVAL_HIST_BINS; ++i) n += hist[i];
    if (n == 0) return NAN;
    for (int i = 0; i < S2M2_EVAL_HIST_BINS; ++i) {
        cum += hist[i];
        if ((double)cum >= p * (double)n) return i == S2M2_EVAL_HIST_BINS - 1 ? INFINITY : (double)(i + 1) / 64.0;
    }
    return INFINITY;
}

// --metrics: `words` = the B stat blocks of s2m2_disp_eval for ground truths of gt_h x g.w pixels
inline bool write_metrics(const char* path, int B, int gt_h, const GroundTruth& g, const Options& o, const unsigned long long* words) {
    FILE* f = fopen(path, "w");
    if (!f) return false;
    fprintf(f, "{\"B\": %d, \"H\": %d, \"W\": %d, \"gt_min\": ", B, gt_h, g.w);
    if (isfinite(o.gt_min)) fprintf(f, "%.9g", o.gt_min);
    else fprintf(f, "null");
    fprintf(f, ", \"conf_min\": %.9g, \"occ_min\": %.9g, \"thresholds\": [", o.conf_min, o.occ_min);
    for (int t = 0; t < g.nthr; ++t) fprintf(f, "%s%.9g", t ? ", " : "", (double)g.thr[t]);
    fprintf(f, "],\n \"pairs\": [");
    for (int b = 0; b < B; ++b) {
        const unsigned long long* w = words + (size_t)b * S2M2_EVAL_WORDS;
        fprintf(f, "%s\n  {", b ? "," : "");
        json_block(f, w + S2M2_EVAL_ALL, g.thr, g.nthr);
        fprintf(f, ", ");
        json_number(f, "a50", eval_quantile(w + S2M2_EVAL_HIST, 0.5), ", ");
        json_number(f, "a90", eval_quantile(w + S2M2_EVAL_HIST, 0.9), ", ");
        json_number(f, "a95", eval_quantile(w + S2M2_EVAL_HIST, 0.95), ", ");
        json_number(f, "a99", eval_quantile(w + S2M2_EVAL_HIST, 0.99), ", ");
        json_number(f, "density", (double)w[S2M2_EVAL_KEPT + S2M2_EVAL_N_EVAL] / (double)w[S2M2_EVAL_ALL + S2M2_EVAL_N_EVAL], ",\n   ");
        fprintf(f, "\"kept\": {");
        json_block(f, w + S2M2_EVAL_KEPT, g.thr, g.nthr);
        fprintf(f, "},\n   \"words\": [");
        for (int i = 0; i < S2M2_EVAL_WORDS; ++i) fprintf(f, "%s%llu", i ? ", " : "", w[i]);
        fprintf(f, "]}");
    }
    fprintf(f, "\n ]}\n");
    return fclose(f) == 0;
}

#endif  // S2M2_RUNNER_HOST_H
