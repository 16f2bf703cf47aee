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
// --normals OUT.f32 [--normals-image OUT.ppm] [--normals-radius R] [--normals-min-cos X]: the normal map of the disparity map (s2m2_normals),
//   behind --calib: raw float32 (3,H,W) unit normals in the camera frame, towards the camera, 0,0,0 = no normal; --normals-image: the normals as
//   colours in a binary PPM (P6), as --register-image writes one.  The neighbours lie R pixels away (1..8, default 1) and are used where their
//   disparity differs by at most R times --max-jump (default 1) px; a normal is kept where its cosine with the direction to the camera is at
//   least X (default 0).  Honours --depth-trunc, --depth-scale, --conf-min, --occ-min and --unfiltered, comes behind --min-size exactly as --ply
//   does, and names its files like --ply for B > 1.  With --repeat: {"normals_count", "repeat", "normals_us_per_pair"} on a line of its own.
// --smooth R --smooth-sigma-r X --smooth-max-jump X [--smooth-sigma-s X] [--smooth-out OUT.f32]: edge-preserving smoothing of the disparity map
//   (s2m2_smooth), behind --calib and --min-size and in front of every 3D output: --ply, --mesh, --depth, --voxel, --register and --normals
//   read the smoothed map, and with --tsdf-frames every frame is fused and tracked from it.  A bilateral filter over the (2R + 1)^2 window
//   (R in 1..8) with the widths --smooth-sigma-s pixels (default R / 2) and --smooth-sigma-r px of disparity; a neighbour enters where its
//   disparity differs from the pixel's by at most --smooth-max-jump px (inf is allowed).  The last two have no default: they depend on the
//   rig's disparity noise.  --smooth-out: the raw float32 (B,1,Hp,Wp) padded map, -1 = dropped.  With --repeat: {"smooth_kept", "repeat",
//   "smooth_us_per_pair"} on a line of its own.
// --min-size N [--max-jump X] [--labels OUT.i32] [--segment-mask OUT.u8]: the speckle filter (s2m2_segment) behind the forward and in front of
//   every 3D output above: the 4-connected components of the kept pixels whose neighbouring disparities differ by at most X px (the --max-jump
//   of --mesh, default 1), and the disparity map without the components of fewer than N pixels (N >= 1; 1 removes nothing).  Needs --calib;
//   honours --depth-trunc, --depth-scale, --conf-min, --occ-min and --unfiltered.  --ply, --mesh, --depth and --register* then read the
//   filtered map with the filter already applied (unfiltered = 1).  --labels: raw int32 (B,1,H,W), the first raster index of every kept pixel's
//   component, -1 = not kept; --segment-mask: raw uint8 (B,1,H,W), 1 = survives.  With --repeat: {"segment_kept", "segment_components",
//   "segment_surviving", "repeat", "segment_us_per_pair"} on a line of its own.  Without --min-size nothing here happens.
//
// --voxel SIZE --voxel-ply OUT.ply [--voxel-max N]: the point cloud downsampled on a voxel grid (s2m2_voxel) -- one vertex per occupied cell of
//   SIZE (the unit of z: metres with a Middlebury calibration), the centroid and the mean colour of the cell's points, in --ply's layout and
//   file naming.  Needs --calib, honours every option of --ply, comes behind --min-size exactly as --ply does, and may be given next to --ply
//   / --mesh or without them.  --voxel-max: the distinct voxels a pair may have (default: a quarter of the image's pixels); a pair with more
//   fails the run instead of leaving a thinned file.  With --repeat: {"voxel_points", "voxel_kept", "voxel_out_of_range", "repeat",
//   "voxel_us_per_pair"} on a line of its own.
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
//
// A stream of pairs from a moving rig fused into one TSDF volume (s2m2_tsdf_integrate / s2m2_tsdf_extract), a mode of its own:
//   s2m2_run_engine ENGINE --tsdf-frames LIST.txt --tsdf-dims NX,NY,NZ --tsdf-voxel VS --tsdf-origin X,Y,Z [--tsdf-trunc T]
//                   [--tsdf-min-weight N] [--tsdf-carve] --calib calib.txt --tsdf-ply OUT.ply [--tsdf-mesh OUT.ply]
//                   [--tsdf-render POSE [--tsdf-render-depth OUT.f32] [--tsdf-render-image OUT.u8] [--tsdf-render-step X]
//                   [--tsdf-render-min-weight N]] [--tsdf-track [--tsdf-track-iters N] [--tsdf-track-dist D] [--tsdf-poses-out FILE]]
// Every line of LIST names LEFT.f32 RIGHT.f32 IMAGE.u8 (as above; raw uint8 (1,3,H,W) for the colours) and the twelve numbers of the pose
//   [R | t], row-major, world -> camera, t in the unit of z; empty lines and lines that start with # are skipped.  The engine (one pair per run)
//   runs per line and the maps are fused behind it; one extraction follows the last line.  --tsdf-dims: the voxels; --tsdf-voxel: their
//   size and --tsdf-origin the centre of voxel (0,0,0), both in the unit of z; --tsdf-trunc: the truncation distance (default 4 VS);
//   --tsdf-min-weight: the frames a voxel needs to count as observed (default 1); --tsdf-carve: also free space in front of the band is
//   fused.  Honours --depth-trunc, --depth-scale, --conf-min, --occ-min and --unfiltered.  --tsdf-ply: the surface points in --ply's layout.
//   --tsdf-mesh (K25, s2m2_tsdf_mesh): also the surface as a triangle mesh in --mesh's layout, the vertices being --tsdf-ply's points; one
//   call behind the extraction; "tsdf_faces" joins the printed line.
//   --tsdf-render POSE (K26, s2m2_tsdf_raycast): the fused volume seen from POSE, twelve comma-separated numbers [R | t], row-major, world ->
//   camera, through the calib's left intrinsics at the engine's H x W: --tsdf-render-depth, raw float32 (1,1,H,W) z (0: hole), and / or
//   --tsdf-render-image, raw uint8 (1,3,H,W); the rays are sampled every --tsdf-render-step (default T / 2) from 0 to the farthest corner of the
//   grid; --tsdf-render-min-weight: the frames a voxel needs (default --tsdf-min-weight's).  "tsdf_render_pixels" (the covered pixels) joins the
//   printed line.
//   --tsdf-track (K27, s2m2_tsdf_track): only the first line's pose is used as given.  For every later line the volume is rendered (K26) from
//   the previous pose through the calib's left camera at H x W, the frame is tracked against that render from the same pose with
//   --tsdf-track-iters iterations (default 10) and the gate --tsdf-track-dist (default T), and fused with the tracked pose; the twelve numbers
//   of those lines are optional and ignored.  A frame whose last iteration was not accepted is not fused and the previous pose stays.
//   "tsdf_tracked" and "tsdf_lost" join the printed line; --tsdf-poses-out: per frame one line of the twelve numbers and the status.
//   LIST is parsed before the engine is loaded.  Prints {"tsdf_frames", "tsdf_points"} on a line of its own.
#include <hip/hip_runtime.h>

#include <functional>

#include "runner_host.h"

static int fail(const char* what) {
    fprintf(stderr, "s2m2_run_engine: %s\n", what);
    return 1;
}

static int fail_lib(const char* what) {
    fprintf(stderr, "s2m2_run_engine: %s: %s\n", what, s2m2_last_error());
    return 1;
}

#define HIP_OK(x, what)                              \
    do {                                             \
        if ((x) != hipSuccess) return fail(what);    \
    } while (0)

// owns one handle -- a device allocation, the engine, the stream, an event: released on every return path, never copied
template <class T, void (*Release)(T)>
struct Owner {
    T h = nullptr;
    Owner() = default;
    Owner(const Owner&) = delete;
    Owner& operator=(const Owner&) = delete;
    ~Owner() {
        if (h) Release(h);
    }
};

static void release_device(void* p) { (void)hipFree(p); }
static void release_engine(s2m2_engine* e) { (void)s2m2_engine_destroy(e); }
static void release_stream(hipStream_t s) { (void)hipStreamDestroy(s); }
static void release_event(hipEvent_t e) { (void)hipEventDestroy(e); }

struct DeviceBuffer : Owner<void*, release_device> {
    // the factory: 0, or 1 behind the message (like every function below that returns int)
    static int make(DeviceBuffer& b, size_t bytes) {
        HIP_OK(hipMalloc(&b.h, bytes), "hipMalloc");
        return 0;
    }
    template <class T>
    T* as() const { return static_cast<T*>(h); }
};

// the milliseconds that `repeat` calls take on the stream: event, calls, event, synchronise (`what` in a message) -- nothing else sits
// between the two events.  `call` returns 0 or reports its own failure
static int time_calls(hipStream_t s, int repeat, const std::function<int()>& call, float* ms, const char* what) {
    Owner<hipEvent_t, release_event> t0, t1;
    HIP_OK(hipEventCreate(&t0.h), "hipEventCreate");
    HIP_OK(hipEventCreate(&t1.h), "hipEventCreate");
    HIP_OK(hipEventRecord(t0.h, s), "hipEventRecord");
    for (int i = 0; i < repeat; ++i)
        if (call() != 0) return 1;
    HIP_OK(hipEventRecord(t1.h, s), "hipEventRecord");
    HIP_OK(hipEventSynchronize(t1.h), what);
    HIP_OK(hipEventElapsedTime(ms, t0.h, t1.h), "hipEventElapsedTime");
    return 0;
}

// one raw output: `bytes` of device memory -> the file `path`; parts > 1: its equal parts -> pair_path(path, parts, b, ext)
static int download_and_write(const void* dev, size_t bytes, const std::string& path, const char* cannot, int parts = 1, const char* ext = "") {
    std::vector<unsigned char> h(bytes);
    HIP_OK(hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost), "download");
    for (int b = 0; b < parts; ++b)
        if (!write_bytes(pair_path(path.c_str(), parts, b, ext), "", h.data() + b * (bytes / parts), bytes / parts)) return fail(cannot);
    return 0;
}

// what every stage behind the forward works on
struct Context {
    const Options& o;
    s2m2_engine_info m;
    const float* maps[3] = {nullptr, nullptr, nullptr};   // disp, occ, conf of the run, on the device
    const void* left = nullptr;                           // the float32 LEFT input, on the device
    hipStream_t s = nullptr;
    Calib cal;                                            // read once, in front of the first 3D stage
    // --min-size: the 3D outputs read the map K22 leaves (`filtered`), with the filter already applied
    const float* disp3d = nullptr;
    int unfiltered3d = 0;
    DeviceBuffer filtered, image;                         // image: --image, uploaded on first use
    DeviceBuffer smoothed;                                // --smooth: the map K29 leaves, behind --min-size's
    explicit Context(const Options& opt) : o(opt) {}
};

// the image the 3D stages take colours from: --image (read and uploaded once, then shared) or the float32 LEFT input
static int left_image(Context& c, const void** image, int* dtype) {
    *image = c.left;
    *dtype = S2M2_F32;
    if (!c.o.image_path) return 0;
    if (!c.image.h) {
        std::vector<unsigned char> hi((size_t)c.m.B * 3 * c.m.H * c.m.W);
        if (!read_raw_u8(c.o.image_path, hi)) {
            fprintf(stderr, "s2m2_run_engine: --image must be a raw uint8 (%d,3,%d,%d) file\n", c.m.B, c.m.H, c.m.W);
            return 1;
        }
        if (DeviceBuffer::make(c.image, hi.size())) return 1;
        HIP_OK(hipMemcpy(c.image.h, hi.data(), hi.size(), hipMemcpyHostToDevice), "upload");
    }
    *image = c.image.h;
    *dtype = 2;
    return 0;
}

// --min-size (K22): the labels, the mask and the filtered map for the stages behind
static int stage_segment(Context& c) {
    const Options& o = c.o;
    const s2m2_engine_info& m = c.m;
    const size_t npix = (size_t)m.H * m.W, map = (size_t)m.B * m.out_h * m.out_w;
    const size_t ws_bytes = s2m2_segment_workspace_bytes(m.B, m.H, m.W);
    if (ws_bytes == 0) return fail("--min-size: extents too large");
    DeviceBuffer dws, dstats, dlabel, dmask;
    if (DeviceBuffer::make(dws, ws_bytes) || DeviceBuffer::make(c.filtered, map * sizeof(float)) ||
        DeviceBuffer::make(dstats, m.B * 4 * sizeof(int32_t)))
        return 1;
    if (o.labels_path && DeviceBuffer::make(dlabel, (size_t)m.B * npix * sizeof(int32_t))) return 1;
    if (o.segmask_path && DeviceBuffer::make(dmask, (size_t)m.B * npix)) return 1;
    s2m2_segment_desc sd;
    memset(&sd, 0, sizeof sd);
    fill_cloud_inputs(sd.cloud, m, c.maps[0], c.maps[1], c.maps[2], nullptr, S2M2_F32, o.unfiltered, c.cal, o);
    sd.label = dlabel.as<int32_t>(); sd.mask = dmask.as<unsigned char>(); sd.disp_out = c.filtered.as<float>();
    sd.stats = dstats.as<int32_t>(); sd.workspace = dws.h;
    sd.max_jump = o.max_jump; sd.min_size = o.min_size;
    const auto run = [&] { return s2m2_segment(&sd, c.s) == 0 ? 0 : fail_lib("s2m2_segment failed"); };
    if (run()) return 1;
    HIP_OK(hipStreamSynchronize(c.s), "s2m2_segment");
    std::vector<int32_t> hstats((size_t)m.B * 4);
    HIP_OK(hipMemcpy(hstats.data(), dstats.h, hstats.size() * sizeof(int32_t), hipMemcpyDeviceToHost), "download");
    if (o.labels_path && download_and_write(dlabel.h, (size_t)m.B * npix * sizeof(int32_t), o.labels_path, "cannot write the labels")) return 1;
    if (o.segmask_path && download_and_write(dmask.h, (size_t)m.B * npix, o.segmask_path, "cannot write the segment mask")) return 1;
    if (o.repeat > 0) {
        float ms = 0.f;
        if (time_calls(c.s, o.repeat, run, &ms, "timed segment runs")) return 1;
        printf("{\"segment_kept\": %d, \"segment_components\": %d, \"segment_surviving\": %d, \"repeat\": %d, \"segment_us_per_pair\": %.2f}\n",
               hstats[0], hstats[1], hstats[2], o.repeat, 1000.f * ms / o.repeat / m.B);
    }
    c.disp3d = c.filtered.as<float>();
    c.unfiltered3d = 1;
    return 0;
}

// the descriptor of --smooth (K29) on the maps disp / occ / conf, into `out`
static void fill_smooth(s2m2_smooth_desc& sd, const s2m2_engine_info& m, const float* disp, const float* occ, const float* conf, int unfiltered,
                        const Calib& cal, const Options& o, float* out, int32_t* count) {
    memset(&sd, 0, sizeof sd);
    fill_cloud_inputs(sd.cloud, m, disp, occ, conf, nullptr, S2M2_F32, unfiltered, cal, o);
    sd.disp_out = out; sd.count = count;
    sd.radius = o.smooth_radius; sd.sigma_s = o.smooth_sigma_s; sd.sigma_r = o.smooth_sigma_r; sd.max_jump = o.smooth_max_jump;
}

// --smooth (K29): the smoothed map for the stages behind, which read it with the filter already applied
static int stage_smooth(Context& c) {
    const Options& o = c.o;
    const s2m2_engine_info& m = c.m;
    const size_t map = (size_t)m.B * m.out_h * m.out_w;
    DeviceBuffer dcount;
    if (DeviceBuffer::make(c.smoothed, map * sizeof(float)) || DeviceBuffer::make(dcount, m.B * sizeof(int32_t))) return 1;
    s2m2_smooth_desc sd;
    fill_smooth(sd, m, c.disp3d, c.maps[1], c.maps[2], c.unfiltered3d, c.cal, o, c.smoothed.as<float>(), dcount.as<int32_t>());
    const auto run = [&] { return s2m2_smooth(&sd, c.s) == 0 ? 0 : fail_lib("s2m2_smooth failed"); };
    if (run()) return 1;
    HIP_OK(hipStreamSynchronize(c.s), "s2m2_smooth");
    std::vector<int32_t> hcount(m.B);
    HIP_OK(hipMemcpy(hcount.data(), dcount.h, m.B * sizeof(int32_t), hipMemcpyDeviceToHost), "download");
    if (o.smooth_out_path && download_and_write(c.smoothed.h, map * sizeof(float), o.smooth_out_path, "cannot write the smoothed map")) return 1;
    if (o.repeat > 0) {
        float ms = 0.f;
        if (time_calls(c.s, o.repeat, run, &ms, "timed smooth runs")) return 1;
        printf("{\"smooth_kept\": %d, \"repeat\": %d, \"smooth_us_per_pair\": %.2f}\n", hcount[0], o.repeat, 1000.f * ms / o.repeat / m.B);
    }
    c.disp3d = c.smoothed.as<float>();
    c.unfiltered3d = 1;
    return 0;
}

// --ply / --mesh / --depth (K15, K20): with --mesh one s2m2_mesh call writes the vertices (the --ply records) and the faces
static int stage_cloud(Context& c) {
    const Options& o = c.o;
    const s2m2_engine_info& m = c.m;
    const size_t npix = (size_t)m.H * m.W;
    const long long fcap = 2LL * (m.H - 1) * (m.W - 1);
    const void* image = nullptr;
    int image_dtype = 0;
    if (left_image(c, &image, &image_dtype)) return 1;
    const size_t ws_bytes = o.mesh_path ? s2m2_mesh_workspace_bytes(m.B, m.H, m.W) : s2m2_cloud_workspace_bytes(m.B, m.H, m.W);
    if (ws_bytes == 0) return fail("the 3D outputs: extents too large");
    DeviceBuffer dfaces, dfcount, drec, dws, dcount, ddepth;
    if (o.mesh_path && (DeviceBuffer::make(dfaces, (size_t)m.B * (fcap > 0 ? fcap : 1) * 12) || DeviceBuffer::make(dfcount, m.B * sizeof(int32_t))))
        return 1;
    if (DeviceBuffer::make(drec, (size_t)m.B * npix * 16) || DeviceBuffer::make(dws, ws_bytes) || DeviceBuffer::make(dcount, m.B * sizeof(int32_t)))
        return 1;
    if (o.depth_path && DeviceBuffer::make(ddepth, (size_t)m.B * npix * sizeof(float))) return 1;
    s2m2_mesh_desc md;
    memset(&md, 0, sizeof md);
    s2m2_cloud_desc& cd = md.cloud;
    fill_cloud_inputs(cd, m, c.disp3d, c.maps[1], c.maps[2], image, image_dtype, c.unfiltered3d, c.cal, o);
    cd.depth = ddepth.as<float>(); cd.records = drec.h; cd.count = dcount.as<int32_t>(); cd.workspace = dws.h;
    cd.capacity = (long long)npix;
    md.faces = dfaces.h; md.face_count = dfcount.as<int32_t>(); md.face_capacity = fcap; md.max_jump = o.max_jump;
    const auto run_mesh = [&] { return s2m2_mesh(&md, c.s) == 0 ? 0 : fail_lib("s2m2_mesh failed"); };
    const auto run_cloud = [&] { return s2m2_cloud(&cd, c.s) == 0 ? 0 : fail_lib("s2m2_cloud failed"); };
    if (o.mesh_path ? run_mesh() : run_cloud()) return 1;
    HIP_OK(hipStreamSynchronize(c.s), "s2m2_cloud");
    std::vector<int32_t> hcount(m.B), hfcount(m.B, 0);
    HIP_OK(hipMemcpy(hcount.data(), dcount.h, m.B * sizeof(int32_t), hipMemcpyDeviceToHost), "download");
    if (o.mesh_path) HIP_OK(hipMemcpy(hfcount.data(), dfcount.h, m.B * sizeof(int32_t), hipMemcpyDeviceToHost), "download");
    std::vector<unsigned char> hrec;
    std::vector<int32_t> hfaces;
    for (int b = 0; b < m.B; ++b) {
        hrec.resize((size_t)hcount[b] * 16);
        HIP_OK(hipMemcpy(hrec.data(), drec.as<char>() + (size_t)b * npix * 16, hrec.size(), hipMemcpyDeviceToHost), "download");
        if (o.ply_path && !write_ply(pair_path(o.ply_path, m.B, b), hrec.data(), hcount[b])) return fail("cannot write the PLY file");
        if (o.mesh_path) {
            hfaces.resize((size_t)hfcount[b] * 3);
            HIP_OK(hipMemcpy(hfaces.data(), dfaces.as<char>() + (size_t)b * fcap * 12, hfaces.size() * 4, hipMemcpyDeviceToHost), "download");
            if (!write_ply_mesh(pair_path(o.mesh_path, m.B, b), hrec.data(), hcount[b], hfaces.data(), hfcount[b]))
                return fail("cannot write the mesh PLY file");
        }
    }
    if (o.depth_path && download_and_write(ddepth.h, (size_t)m.B * npix * sizeof(float), o.depth_path, "cannot write the depth map")) return 1;
    float ms = 0.f;
    if (o.repeat > 0 && o.mesh_path) {
        if (time_calls(c.s, o.repeat, run_mesh, &ms, "timed mesh runs")) return 1;
        printf("{\"mesh_vertices\": %d, \"mesh_faces\": %d, \"repeat\": %d, \"mesh_us_per_pair\": %.2f}\n", hcount[0], hfcount[0], o.repeat,
               1000.f * ms / o.repeat / m.B);
    }
    if (o.repeat > 0 && o.ply_path) {
        if (time_calls(c.s, o.repeat, run_cloud, &ms, "timed cloud runs")) return 1;
        printf("{\"cloud_points\": %d, \"repeat\": %d, \"cloud_us_per_pair\": %.2f}\n", hcount[0], o.repeat, 1000.f * ms / o.repeat / m.B);
    }
    return 0;
}

// --voxel (K23): the downsampled cloud
static int stage_voxel(Context& c) {
    const Options& o = c.o;
    const s2m2_engine_info& m = c.m;
    const size_t npix = (size_t)m.H * m.W;
    const long long max_voxels = o.voxel_max > 0 ? o.voxel_max : (npix / 4 > 0 ? (long long)(npix / 4) : 1);
    const void* image = nullptr;
    int image_dtype = 0;
    if (left_image(c, &image, &image_dtype)) return 1;
    const size_t ws_bytes = s2m2_voxel_workspace_bytes(m.B, m.H, m.W, max_voxels);
    if (ws_bytes == 0) return fail("--voxel: extents or --voxel-max too large");
    DeviceBuffer drec, dws, dcount, dstats;
    if (DeviceBuffer::make(drec, (size_t)m.B * max_voxels * 16) || DeviceBuffer::make(dws, ws_bytes) || DeviceBuffer::make(dcount, m.B * sizeof(int32_t)) ||
        DeviceBuffer::make(dstats, m.B * 4 * sizeof(int32_t)))
        return 1;
    s2m2_voxel_desc vd;
    memset(&vd, 0, sizeof vd);
    fill_cloud_inputs(vd.cloud, m, c.disp3d, c.maps[1], c.maps[2], image, image_dtype, c.unfiltered3d, c.cal, o);
    vd.records = drec.h; vd.count = dcount.as<int32_t>(); vd.stats = dstats.as<int32_t>(); vd.workspace = dws.h;
    vd.voxel_size = o.voxel_size; vd.max_voxels = max_voxels; vd.capacity = max_voxels;
    const auto run = [&] { return s2m2_voxel(&vd, c.s) == 0 ? 0 : fail_lib("s2m2_voxel failed"); };
    if (run()) return 1;
    HIP_OK(hipStreamSynchronize(c.s), "s2m2_voxel");
    std::vector<int32_t> hcount(m.B), hstats((size_t)m.B * 4);
    HIP_OK(hipMemcpy(hcount.data(), dcount.h, m.B * sizeof(int32_t), hipMemcpyDeviceToHost), "download");
    HIP_OK(hipMemcpy(hstats.data(), dstats.h, hstats.size() * sizeof(int32_t), hipMemcpyDeviceToHost), "download");
    std::vector<unsigned char> hrec;
    for (int b = 0; b < m.B; ++b) {
        if (hstats[(size_t)b * 4 + 2] != 0) return fail("--voxel: more voxels than --voxel-max (default: a quarter of the pixels): give a larger one");
        hrec.resize((size_t)hcount[b] * 16);
        HIP_OK(hipMemcpy(hrec.data(), drec.as<char>() + (size_t)b * max_voxels * 16, hrec.size(), hipMemcpyDeviceToHost), "download");
        if (!write_ply(pair_path(o.voxel_ply_path, m.B, b), hrec.data(), hcount[b])) return fail("cannot write the voxel PLY file");
    }
    if (o.repeat > 0) {
        float ms = 0.f;
        if (time_calls(c.s, o.repeat, run, &ms, "timed voxel runs")) return 1;
        printf("{\"voxel_points\": %d, \"voxel_kept\": %d, \"voxel_out_of_range\": %d, \"repeat\": %d, \"voxel_us_per_pair\": %.2f}\n", hcount[0],
               hstats[0], hstats[1], o.repeat, 1000.f * ms / o.repeat / m.B);
    }
    return 0;
}

// --register (K21): the depth map, the winners' indices and their colours in the target camera
static int stage_register(Context& c) {
    const Options& o = c.o;
    const s2m2_engine_info& m = c.m;
    TargetCamera cam;
    if (strcmp(o.register_cam, "right") == 0) {
        if (!c.cal.have_cam1) return fail("--register right: the calib file has no cam1");
        cam.width = m.W; cam.height = m.H;
        cam.fx = c.cal.cam1[0]; cam.fy = c.cal.cam1[1]; cam.cx = c.cal.cam1[2]; cam.cy = c.cal.cam1[3];
        cam.t[0] = -c.cal.baseline / o.depth_scale;
    } else if (!read_camera(o.register_cam, cam)) return fail("--register: the word right, or a file with width=, height= and cam=[fx 0 cx; 0 fy cy; 0 0 1]");
    const size_t ws_bytes = s2m2_register_workspace_bytes(m.B, cam.height, cam.width);
    if (ws_bytes == 0) return fail("--register: target extents too large");
    const size_t tpix = (size_t)cam.height * cam.width;
    const void* image = nullptr;
    int image_dtype = 0;
    if (left_image(c, &image, &image_dtype)) return 1;
    DeviceBuffer dws, dd, dcount, di, dc;
    if (DeviceBuffer::make(dws, ws_bytes) || DeviceBuffer::make(dd, (size_t)m.B * tpix * sizeof(float)) ||
        DeviceBuffer::make(dcount, m.B * sizeof(int32_t)))
        return 1;
    if (o.reg_index_path && DeviceBuffer::make(di, (size_t)m.B * tpix * sizeof(int32_t))) return 1;
    if (o.reg_image_path && DeviceBuffer::make(dc, (size_t)m.B * 3 * tpix)) return 1;
    s2m2_register_desc rd;
    memset(&rd, 0, sizeof rd);
    fill_cloud_inputs(rd.cloud, m, c.disp3d, c.maps[1], c.maps[2], image, image_dtype, c.unfiltered3d, c.cal, o);
    rd.Ht = cam.height; rd.Wt = cam.width; rd.splat = o.splat;
    rd.fx_t = cam.fx; rd.fy_t = cam.fy; rd.cx_t = cam.cx; rd.cy_t = cam.cy;
    memcpy(rd.R, cam.R, sizeof rd.R);
    memcpy(rd.t, cam.t, sizeof rd.t);
    rd.depth_t = dd.as<float>(); rd.index_t = di.as<int32_t>(); rd.image_t = dc.as<unsigned char>();
    rd.count = dcount.as<int32_t>(); rd.workspace = dws.h;
    const auto run = [&] { return s2m2_register(&rd, c.s) == 0 ? 0 : fail_lib("s2m2_register failed"); };
    if (run()) return 1;
    HIP_OK(hipStreamSynchronize(c.s), "s2m2_register");
    std::vector<int32_t> hcount(m.B);
    HIP_OK(hipMemcpy(hcount.data(), dcount.h, m.B * sizeof(int32_t), hipMemcpyDeviceToHost), "download");
    if (download_and_write(dd.h, (size_t)m.B * tpix * sizeof(float), o.reg_depth_path, "cannot write the registered depth map", m.B, ".f32")) return 1;
    if (o.reg_index_path &&
        download_and_write(di.h, (size_t)m.B * tpix * sizeof(int32_t), o.reg_index_path, "cannot write the registered index map", m.B, ".i32"))
        return 1;
    if (o.reg_image_path) {
        std::vector<unsigned char> planar((size_t)m.B * 3 * tpix), rgb(3 * tpix);
        HIP_OK(hipMemcpy(planar.data(), dc.h, planar.size(), hipMemcpyDeviceToHost), "download");
        char head[64];
        snprintf(head, sizeof head, "P6\n%d %d\n255\n", cam.width, cam.height);
        for (int b = 0; b < m.B; ++b) {
            for (size_t i = 0; i < tpix; ++i)
                for (int ch = 0; ch < 3; ++ch) rgb[3 * i + ch] = planar[((size_t)b * 3 + ch) * tpix + i];
            if (!write_bytes(pair_path(o.reg_image_path, m.B, b, ".ppm"), head, rgb.data(), rgb.size())) return fail("cannot write the registered image");
        }
    }
    if (o.repeat > 0) {
        float ms = 0.f;
        if (time_calls(c.s, o.repeat, run, &ms, "timed register runs")) return 1;
        printf("{\"register_covered\": %d, \"repeat\": %d, \"register_us_per_pair\": %.2f}\n", hcount[0], o.repeat, 1000.f * ms / o.repeat / m.B);
    }
    return 0;
}

// --normals (K28): the normal map of the run's own maps, and the normals as colours
static int stage_normals(Context& c) {
    const Options& o = c.o;
    const s2m2_engine_info& m = c.m;
    const size_t npix = (size_t)m.H * m.W;
    DeviceBuffer dn, dcount, dc;
    if (DeviceBuffer::make(dn, (size_t)m.B * 3 * npix * sizeof(float)) || DeviceBuffer::make(dcount, m.B * sizeof(int32_t))) return 1;
    if (o.normals_image_path && DeviceBuffer::make(dc, (size_t)m.B * 3 * npix)) return 1;
    s2m2_normals_desc nd;
    memset(&nd, 0, sizeof nd);
    fill_cloud_inputs(nd.cloud, m, c.disp3d, c.maps[1], c.maps[2], nullptr, 2, c.unfiltered3d, c.cal, o);
    nd.normals = dn.as<float>(); nd.image = dc.as<unsigned char>(); nd.count = dcount.as<int32_t>();
    nd.radius = o.normals_radius; nd.max_jump = o.max_jump; nd.min_cos = o.normals_min_cos;
    const auto run = [&] { return s2m2_normals(&nd, c.s) == 0 ? 0 : fail_lib("s2m2_normals failed"); };
    if (run()) return 1;
    HIP_OK(hipStreamSynchronize(c.s), "s2m2_normals");
    std::vector<int32_t> hcount(m.B);
    HIP_OK(hipMemcpy(hcount.data(), dcount.h, m.B * sizeof(int32_t), hipMemcpyDeviceToHost), "download");
    if (download_and_write(dn.h, (size_t)m.B * 3 * npix * sizeof(float), o.normals_path, "cannot write the normal map", m.B, ".f32")) return 1;
    if (o.normals_image_path) {
        std::vector<unsigned char> planar((size_t)m.B * 3 * npix), rgb(3 * npix);
        HIP_OK(hipMemcpy(planar.data(), dc.h, planar.size(), hipMemcpyDeviceToHost), "download");
        char head[64];
        snprintf(head, sizeof head, "P6\n%d %d\n255\n", m.W, m.H);
        for (int b = 0; b < m.B; ++b) {
            for (size_t i = 0; i < npix; ++i)
                for (int ch = 0; ch < 3; ++ch) rgb[3 * i + ch] = planar[((size_t)b * 3 + ch) * npix + i];
            if (!write_bytes(pair_path(o.normals_image_path, m.B, b, ".ppm"), head, rgb.data(), rgb.size())) return fail("cannot write the normal image");
        }
    }
    if (o.repeat > 0) {
        float ms = 0.f;
        if (time_calls(c.s, o.repeat, run, &ms, "timed normals runs")) return 1;
        printf("{\"normals_count\": %d, \"repeat\": %d, \"normals_us_per_pair\": %.2f}\n", hcount[0], o.repeat, 1000.f * ms / o.repeat / m.B);
    }
    return 0;
}

// --gt (K18): the stat words of every pair and the numbers derived from them, as JSON
static int stage_eval(Context& c, const GroundTruth& g) {
    const Options& o = c.o;
    const s2m2_engine_info& m = c.m;
    const int gt_h = g.rows / m.B;
    const size_t ws_bytes = s2m2_eval_workspace_bytes(m.B, gt_h, g.w), nwords = (size_t)m.B * S2M2_EVAL_WORDS;
    if (ws_bytes == 0) return fail("--gt: extents too large");
    DeviceBuffer dgt, dregion, dws, dstats;
    if (DeviceBuffer::make(dgt, g.gt.size() * sizeof(float))) return 1;
    HIP_OK(hipMemcpy(dgt.h, g.gt.data(), g.gt.size() * sizeof(float), hipMemcpyHostToDevice), "upload");
    if (o.region_path) {
        if (DeviceBuffer::make(dregion, g.region.size())) return 1;
        HIP_OK(hipMemcpy(dregion.h, g.region.data(), g.region.size(), hipMemcpyHostToDevice), "upload");
    }
    if (DeviceBuffer::make(dws, ws_bytes) || DeviceBuffer::make(dstats, nwords * sizeof(unsigned long long))) return 1;
    s2m2_eval_desc ed;
    memset(&ed, 0, sizeof ed);
    ed.disp = c.maps[0]; ed.occ = c.maps[1]; ed.conf = c.maps[2];
    ed.gt = dgt.as<float>(); ed.region = dregion.as<unsigned char>(); ed.workspace = dws.h; ed.stats = dstats.as<unsigned long long>();
    ed.B = m.B; ed.H = gt_h; ed.W = g.w; ed.Hp = m.out_h; ed.Wp = m.out_w;
    ed.nthr = g.nthr;
    for (int t = 0; t < g.nthr; ++t) ed.thr[t] = g.thr[t];
    ed.d1_abs = 3.f; ed.d1_rel = 0.05f;
    ed.gt_min = (float)o.gt_min; ed.conf_min = (float)o.conf_min; ed.occ_min = (float)o.occ_min;
    const auto run = [&] { return s2m2_disp_eval(&ed, c.s) == 0 ? 0 : fail_lib("s2m2_disp_eval failed"); };
    if (run()) return 1;
    HIP_OK(hipStreamSynchronize(c.s), "s2m2_disp_eval");
    std::vector<unsigned long long> hs(nwords);
    HIP_OK(hipMemcpy(hs.data(), dstats.h, nwords * sizeof(unsigned long long), hipMemcpyDeviceToHost), "download");
    if (!write_metrics(o.metrics_path, m.B, gt_h, g, o, hs.data())) return fail("cannot write the metrics");
    if (o.repeat > 0) {
        float ms = 0.f;
        if (time_calls(c.s, o.repeat, run, &ms, "timed evaluation runs")) return 1;
        printf("{\"eval_pixels\": %llu, \"repeat\": %d, \"eval_us_per_pair\": %.2f}\n", hs[S2M2_EVAL_N_EVAL], o.repeat, 1000.f * ms / o.repeat / m.B);
    }
    return 0;
}

// --tsdf-render (K26): the volume seen from the option's pose through the calib's left camera at H x W -> the covered pixels in `pixels`
static int render_tsdf(const Options& o, const s2m2_engine_info& m, const Calib& cal, const void* volume, hipStream_t s, int32_t& pixels) {
    const size_t plane = (size_t)m.H * m.W;
    DeviceBuffer dpose, ddepth, dimage, dcount;
    if (DeviceBuffer::make(dpose, sizeof o.tsdf_render_pose) || DeviceBuffer::make(dcount, sizeof(int32_t)) ||
        (o.tsdf_render_depth_path && DeviceBuffer::make(ddepth, plane * sizeof(float))) || (o.tsdf_render_image_path && DeviceBuffer::make(dimage, 3 * plane)))
        return 1;
    HIP_OK(hipMemcpy(dpose.h, o.tsdf_render_pose, sizeof o.tsdf_render_pose, hipMemcpyHostToDevice), "upload");
    s2m2_tsdf_raycast_desc rd;
    memset(&rd, 0, sizeof rd);
    rd.volume = volume; rd.poses = dpose.as<float>();
    rd.depth = o.tsdf_render_depth_path ? ddepth.as<float>() : nullptr;
    rd.image = o.tsdf_render_image_path ? dimage.as<uint8_t>() : nullptr;
    rd.count = dcount.as<int32_t>();
    rd.B = 1; rd.Ht = m.H; rd.Wt = m.W;
    rd.Nx = o.tsdf_dims[0]; rd.Ny = o.tsdf_dims[1]; rd.Nz = o.tsdf_dims[2];
    rd.min_weight = o.tsdf_render_min_weight;
    rd.fx = cal.fx; rd.fy = cal.fy; rd.cx = cal.cx; rd.cy = cal.cy;
    memcpy(rd.origin, o.tsdf_origin, sizeof rd.origin);
    rd.voxel_size = o.tsdf_voxel;
    rd.z_near = 0.0; rd.z_far = tsdf_far_corner(o.tsdf_render_pose, o.tsdf_dims, o.tsdf_origin, o.tsdf_voxel); rd.step = o.tsdf_render_step;
    if (s2m2_tsdf_raycast(&rd, s) != 0) return fail_lib("s2m2_tsdf_raycast failed");
    HIP_OK(hipStreamSynchronize(s), "s2m2_tsdf_raycast");
    HIP_OK(hipMemcpy(&pixels, dcount.h, sizeof pixels, hipMemcpyDeviceToHost), "download");
    if (o.tsdf_render_depth_path) {
        std::vector<float> h(plane);
        HIP_OK(hipMemcpy(h.data(), ddepth.h, plane * sizeof(float), hipMemcpyDeviceToHost), "download");
        if (!write_bytes(o.tsdf_render_depth_path, "", h.data(), plane * sizeof(float))) return fail("cannot write the --tsdf-render-depth file");
    }
    if (o.tsdf_render_image_path) {
        std::vector<unsigned char> h(3 * plane);
        HIP_OK(hipMemcpy(h.data(), dimage.h, 3 * plane, hipMemcpyDeviceToHost), "download");
        if (!write_bytes(o.tsdf_render_image_path, "", h.data(), 3 * plane)) return fail("cannot write the --tsdf-render-image file");
    }
    return 0;
}

// --tsdf-track (K27): what a tracked frame needs beside the fusion's buffers, and the step itself
struct Tracker {
    DeviceBuffer model_pose, depth, gradients, systems, workspace;
    s2m2_tsdf_raycast_desc rd;
    s2m2_tsdf_track_desc kd;
    int n_iters = 0;

    int make(const Options& o, const s2m2_engine_info& m, const Calib& cal, const s2m2_tsdf_desc& td) {
        const size_t plane = (size_t)m.H * m.W, ws = s2m2_tsdf_track_workspace_bytes(1, m.H, m.W);
        n_iters = o.tsdf_track_iters;
        if (ws == 0) return fail("--tsdf-track: the image is too large");
        if (DeviceBuffer::make(model_pose, 12 * sizeof(float)) || DeviceBuffer::make(depth, plane * sizeof(float)) ||
            DeviceBuffer::make(gradients, 3 * plane * sizeof(float)) || DeviceBuffer::make(systems, (size_t)n_iters * 32 * sizeof(double)) ||
            DeviceBuffer::make(workspace, ws))
            return 1;
        memset(&rd, 0, sizeof rd);
        rd.volume = td.volume; rd.poses = model_pose.as<float>();
        rd.depth = depth.as<float>(); rd.gradients = gradients.as<float>();
        rd.B = 1; rd.Ht = m.H; rd.Wt = m.W;
        rd.Nx = td.Nx; rd.Ny = td.Ny; rd.Nz = td.Nz;
        rd.min_weight = o.tsdf_min_weight;
        rd.fx = cal.fx; rd.fy = cal.fy; rd.cx = cal.cx; rd.cy = cal.cy;
        memcpy(rd.origin, td.origin, sizeof rd.origin);
        rd.voxel_size = td.voxel_size;
        rd.z_near = 0.0; rd.step = 0.5 * td.trunc;
        memset(&kd, 0, sizeof kd);
        kd.cloud = td.cloud;
        kd.poses = const_cast<float*>(td.poses); kd.model_poses = model_pose.as<float>();
        kd.model_depth = depth.as<float>(); kd.model_gradients = gradients.as<float>();
        kd.systems = systems.as<double>(); kd.workspace = workspace.h;
        kd.Ht = m.H; kd.Wt = m.W;
        kd.min_count = 100; kd.n_iters = n_iters;
        kd.mfx = cal.fx; kd.mfy = cal.fy; kd.mcx = cal.cx; kd.mcy = cal.cy;
        kd.max_dist = o.tsdf_track_dist; kd.max_rot = 0.2; kd.max_trans = 4.0 * td.trunc;
        return 0;
    }

    // the frame whose maps the engine just wrote, from `pose` (the previous frame's): the refined pose stays in the fusion's pose buffer and
    // comes back in `pose` where the last iteration was accepted -> its status in `status`
    int step(const Options& o, float* pose, hipStream_t s, int& status) {
        HIP_OK(hipMemcpy(model_pose.h, pose, 12 * sizeof(float), hipMemcpyHostToDevice), "upload");
        HIP_OK(hipMemcpy(kd.poses, pose, 12 * sizeof(float), hipMemcpyHostToDevice), "upload");
        rd.z_far = tsdf_far_corner(pose, o.tsdf_dims, o.tsdf_origin, o.tsdf_voxel);
        if (s2m2_tsdf_raycast(&rd, s) != 0) return fail_lib("s2m2_tsdf_raycast failed");
        if (s2m2_tsdf_track(&kd, s) != 0) return fail_lib("s2m2_tsdf_track failed");
        HIP_OK(hipStreamSynchronize(s), "s2m2_tsdf_track");
        double row[32];
        HIP_OK(hipMemcpy(row, systems.as<double>() + (size_t)(n_iters - 1) * 32, sizeof row, hipMemcpyDeviceToHost), "download");
        status = (int)row[29];
        if (status == 0) HIP_OK(hipMemcpy(pose, kd.poses, 12 * sizeof(float), hipMemcpyDeviceToHost), "download");
        return 0;
    }
};

// --tsdf-frames (K24): the engine per line of LIST, the maps fused into the volume behind it, one extraction at the end
static int run_tsdf(const Options& o, s2m2_engine* eng, const s2m2_engine_info& m, const std::vector<TsdfFrame>& frames, hipStream_t s) {
    if (m.B != 1) return fail("--tsdf-frames needs an engine of one pair per run");
    if (m.out_h != m.H || m.out_w != m.W) return fail("the 3D outputs need maps of the image's size (an engine without output_upsample)");
    Calib cal;
    if (!read_calib(o.calib_path, cal)) return fail("--calib: cannot read cam0 and baseline from the file");
    const size_t img = (size_t)3 * m.H * m.W, map = (size_t)m.out_h * m.out_w;
    const size_t voxels = (size_t)o.tsdf_dims[0] * o.tsdf_dims[1] * o.tsdf_dims[2];
    const size_t ws_bytes = s2m2_tsdf_workspace_bytes(o.tsdf_dims[0], o.tsdf_dims[1], o.tsdf_dims[2]);
    if (ws_bytes == 0) return fail("--tsdf-dims: too large");
    DeviceBuffer dl, dr, dimage, dout[3], dvol, dpose, dws, dcount, drec;
    if (DeviceBuffer::make(dl, img * sizeof(float)) || DeviceBuffer::make(dr, img * sizeof(float)) || DeviceBuffer::make(dimage, img) ||
        DeviceBuffer::make(dvol, voxels * 16) || DeviceBuffer::make(dpose, 12 * sizeof(float)) || DeviceBuffer::make(dws, ws_bytes) ||
        DeviceBuffer::make(dcount, sizeof(int32_t)))
        return 1;
    for (auto& p : dout)
        if (DeviceBuffer::make(p, map * sizeof(float))) return 1;
    HIP_OK(hipMemsetAsync(dvol.h, 0, voxels * 16, s), "hipMemsetAsync");
    s2m2_tsdf_desc td;
    memset(&td, 0, sizeof td);
    fill_cloud_inputs(td.cloud, m, dout[0].as<float>(), dout[1].as<float>(), dout[2].as<float>(), dimage.h, 2, o.unfiltered, cal, o);
    DeviceBuffer dsmooth;                                                    // --smooth (K29): every frame is fused, and tracked, from its smoothed map
    s2m2_smooth_desc sm;
    if (o.smooth_arg) {
        if (DeviceBuffer::make(dsmooth, map * sizeof(float))) return 1;
        fill_smooth(sm, m, dout[0].as<float>(), dout[1].as<float>(), dout[2].as<float>(), o.unfiltered, cal, o, dsmooth.as<float>(), nullptr);
        td.cloud.disp = dsmooth.as<float>();
        td.cloud.unfiltered = 1;
    }
    td.volume = dvol.h; td.poses = dpose.as<float>();
    td.Nx = o.tsdf_dims[0]; td.Ny = o.tsdf_dims[1]; td.Nz = o.tsdf_dims[2];
    td.max_weight = 32767; td.carve = o.tsdf_carve;
    memcpy(td.origin, o.tsdf_origin, sizeof td.origin);
    td.voxel_size = o.tsdf_voxel; td.trunc = o.tsdf_trunc;
    Tracker tracker;
    if (o.tsdf_track && tracker.make(o, m, cal, td)) return 1;
    float pose[12];                                                          // --tsdf-track: the pose of the last frame that was fused
    int tracked = 0, lost = 0;
    std::string poses_out;
    std::vector<float> hl(img), hr(img);
    std::vector<unsigned char> hi(img);
    for (const TsdfFrame& fr : frames) {
        const bool first = &fr == &frames[0];
        if (!read_raw(fr.left.c_str(), hl) || !read_raw(fr.right.c_str(), hr) || !read_raw_u8(fr.image.c_str(), hi)) {
            fprintf(stderr, "s2m2_run_engine: --tsdf-frames: %s and %s must be raw float32 and %s raw uint8 (1,3,%d,%d) files\n", fr.left.c_str(),
                    fr.right.c_str(), fr.image.c_str(), m.H, m.W);
            return 1;
        }
        HIP_OK(hipMemcpy(dl.h, hl.data(), img * sizeof(float), hipMemcpyHostToDevice), "upload");
        HIP_OK(hipMemcpy(dr.h, hr.data(), img * sizeof(float), hipMemcpyHostToDevice), "upload");
        HIP_OK(hipMemcpy(dimage.h, hi.data(), img, hipMemcpyHostToDevice), "upload");
        if (!o.tsdf_track || first) HIP_OK(hipMemcpy(dpose.h, fr.pose, sizeof fr.pose, hipMemcpyHostToDevice), "upload");
        if (s2m2_engine_run(eng, dl.h, dr.h, dout[0].as<float>(), dout[1].as<float>(), dout[2].as<float>(), s) != 0) return fail_lib("engine run failed");
        if (o.smooth_arg && s2m2_smooth(&sm, s) != 0) return fail_lib("s2m2_smooth failed");
        int status = 0;
        if (o.tsdf_track && first) memcpy(pose, fr.pose, sizeof pose);
        if (o.tsdf_track && !first) {
            if (int rc = tracker.step(o, pose, s, status)) return rc;
            ++(status == 0 ? tracked : lost);
        }
        if (o.tsdf_track) {
            char num[32];
            for (int i = 0; i < 12; ++i) {
                snprintf(num, sizeof num, "%.9g ", (double)pose[i]);
                poses_out += num;
            }
            poses_out += std::to_string(status) + "\n";
        }
        if (status == 0 && s2m2_tsdf_integrate(&td, s) != 0) return fail_lib("s2m2_tsdf_integrate failed");
        HIP_OK(hipStreamSynchronize(s), "s2m2_tsdf_integrate");       // the next line overwrites the inputs
    }
    if (o.tsdf_poses_out_path && !write_bytes(o.tsdf_poses_out_path, "", poses_out.data(), poses_out.size()))
        return fail("cannot write the --tsdf-poses-out file");
    s2m2_tsdf_extract_desc ed;
    memset(&ed, 0, sizeof ed);
    ed.volume = dvol.h; ed.count = dcount.as<int32_t>(); ed.workspace = dws.h;
    ed.Nx = td.Nx; ed.Ny = td.Ny; ed.Nz = td.Nz; ed.min_weight = o.tsdf_min_weight;
    memcpy(ed.origin, o.tsdf_origin, sizeof ed.origin);
    ed.voxel_size = o.tsdf_voxel;
    int32_t n = 0;                                                           // the count first, then records for exactly that many points
    if (s2m2_tsdf_extract(&ed, s) != 0) return fail_lib("s2m2_tsdf_extract failed");
    HIP_OK(hipStreamSynchronize(s), "s2m2_tsdf_extract");
    HIP_OK(hipMemcpy(&n, dcount.h, sizeof n, hipMemcpyDeviceToHost), "download");
    std::vector<unsigned char> hrec((size_t)n * 16);
    if (n > 0) {
        if (DeviceBuffer::make(drec, hrec.size())) return 1;
        ed.records = drec.h; ed.capacity = n;
        if (s2m2_tsdf_extract(&ed, s) != 0) return fail_lib("s2m2_tsdf_extract failed");
        HIP_OK(hipStreamSynchronize(s), "s2m2_tsdf_extract");
        HIP_OK(hipMemcpy(hrec.data(), drec.h, hrec.size(), hipMemcpyDeviceToHost), "download");
    }
    if (!write_ply(o.tsdf_ply_path, hrec.data(), n)) return fail("cannot write the TSDF PLY file");
    std::string render;                                                      // what --tsdf-render adds to the printed line
    if (o.tsdf_render_arg) {
        int32_t pixels = 0;
        if (int rc = render_tsdf(o, m, cal, dvol.h, s, pixels)) return rc;
        render = ", \"tsdf_render_pixels\": " + std::to_string(pixels);
    }
    if (o.tsdf_track) render += ", \"tsdf_tracked\": " + std::to_string(tracked) + ", \"tsdf_lost\": " + std::to_string(lost);
    if (!o.tsdf_mesh_path) {
        printf("{\"tsdf_frames\": %zu, \"tsdf_points\": %d%s}\n", frames.size(), n, render.c_str());
        return 0;
    }
    // --tsdf-mesh (K25): one faces-only call -- the vertices are the records above.  A face takes three of a cell's points, a cell with p points
    // has at most p - 2 faces and a point lies on the edge of at most four cells: 4 n faces always suffice.
    const size_t mesh_ws_bytes = s2m2_tsdf_mesh_workspace_bytes(td.Nx, td.Ny, td.Nz);
    if (mesh_ws_bytes == 0) return fail("--tsdf-mesh: --tsdf-dims too large");
    const long long fcap = 4LL * n;
    DeviceBuffer dmws, dfaces, dfcount;
    if (DeviceBuffer::make(dmws, mesh_ws_bytes) || DeviceBuffer::make(dfcount, sizeof(int32_t)) ||
        (fcap > 0 && DeviceBuffer::make(dfaces, (size_t)fcap * 3 * sizeof(int32_t))))
        return 1;
    s2m2_tsdf_mesh_desc md;
    memset(&md, 0, sizeof md);
    md.extract = ed;
    md.extract.records = nullptr; md.extract.count = nullptr; md.extract.capacity = 0; md.extract.workspace = dmws.h;
    md.faces = fcap > 0 ? dfaces.h : nullptr; md.face_count = dfcount.as<int32_t>(); md.face_capacity = fcap;
    if (s2m2_tsdf_mesh(&md, s) != 0) return fail_lib("s2m2_tsdf_mesh failed");
    HIP_OK(hipStreamSynchronize(s), "s2m2_tsdf_mesh");
    int32_t nf = 0;
    HIP_OK(hipMemcpy(&nf, dfcount.h, sizeof nf, hipMemcpyDeviceToHost), "download");
    if (nf > fcap) return fail("--tsdf-mesh: more faces than four per point");
    std::vector<int32_t> hfaces((size_t)nf * 3);
    if (nf > 0) HIP_OK(hipMemcpy(hfaces.data(), dfaces.h, hfaces.size() * sizeof(int32_t), hipMemcpyDeviceToHost), "download");
    if (!write_ply_mesh(o.tsdf_mesh_path, hrec.data(), n, hfaces.data(), nf)) return fail("cannot write the TSDF mesh PLY file");
    printf("{\"tsdf_frames\": %zu, \"tsdf_points\": %d, \"tsdf_faces\": %d%s}\n", frames.size(), n, nf, render.c_str());
    return 0;
}

int main(int argc, char** argv) {
    Options o;
    if (!parse_options(argc, argv, o)) return fail(USAGE);
    if (const char* msg = check_options(o)) return fail(msg);
    std::vector<TsdfFrame> tsdf_frames;                   // LIST is parsed here, before the engine is loaded
    if (o.tsdf_frames_path) {
        const std::string msg = read_tsdf_frames(o.tsdf_frames_path, tsdf_frames, o.tsdf_track != 0);
        if (!msg.empty()) return fail(msg.c_str());
    }
    // the ground truth is parsed and validated here, before the engine is loaded and anything touches the device
    GroundTruth g;
    const std::string gt_msg = read_ground_truth(o, g);
    if (!gt_msg.empty()) return fail(gt_msg.c_str());
    if (s2m2_version() != S2M2_ABI_VERSION) return fail("libs2m2_hip.so was built from another ABI version than this program");

    // declared in the reverse of the order of release: the engine goes first, the stream last
    Owner<hipStream_t, release_stream> stream;
    DeviceBuffer dl, dr, dout[3];
    Context c(o);
    Owner<s2m2_engine*, release_engine> eng;
    if (s2m2_engine_load(o.pos[0], &eng.h) != 0) return fail_lib("cannot load the engine");
    s2m2_engine_info& m = c.m;
    s2m2_engine_meta(eng.h, &m);
    if (m.image_dtype != S2M2_F32) return fail("this program feeds float32 images; the engine takes another image dtype");
    if (o.tsdf_frames_path) {
        HIP_OK(hipStreamCreateWithFlags(&stream.h, hipStreamNonBlocking), "hipStreamCreate");
        return run_tsdf(o, eng.h, m, tsdf_frames, stream.h);
    }
    if (o.gt_path && (g.rows % m.B != 0 || g.rows / m.B > m.out_h || g.w > m.out_w)) {
        fprintf(stderr, "s2m2_run_engine: --gt is %d x %d pixels; the engine needs B = %d stacked ground truths of at most %d x %d\n", g.w, g.rows,
                m.B, m.out_w, m.out_h);
        return 1;
    }
    const size_t img = (size_t)m.B * 3 * m.H * m.W, map = (size_t)m.B * m.out_h * m.out_w;
    std::vector<float> hl(img), hr(img);
    if (!read_raw(o.pos[1], hl) || !read_raw(o.pos[2], hr)) {
        fprintf(stderr, "s2m2_run_engine: the images must be raw float32 (%d,3,%d,%d) files\n", m.B, m.H, m.W);
        return 1;
    }
    if (DeviceBuffer::make(dl, img * sizeof(float)) || DeviceBuffer::make(dr, img * sizeof(float))) return 1;
    for (auto& p : dout)
        if (DeviceBuffer::make(p, map * sizeof(float))) return 1;
    HIP_OK(hipMemcpy(dl.h, hl.data(), img * sizeof(float), hipMemcpyHostToDevice), "upload");
    HIP_OK(hipMemcpy(dr.h, hr.data(), img * sizeof(float), hipMemcpyHostToDevice), "upload");
    HIP_OK(hipStreamCreateWithFlags(&stream.h, hipStreamNonBlocking), "hipStreamCreate");
    for (int k = 0; k < 3; ++k) c.maps[k] = dout[k].as<float>();
    c.left = dl.h;
    c.s = stream.h;
    c.disp3d = c.maps[0];
    c.unfiltered3d = o.unfiltered;

    const auto forward = [&] {
        return s2m2_engine_run(eng.h, dl.h, dr.h, dout[0].as<float>(), dout[1].as<float>(), dout[2].as<float>(), c.s) == 0 ? 0 : fail_lib("engine run failed");
    };
    if (forward()) return 1;
    HIP_OK(hipStreamSynchronize(c.s), "engine run");
    if (o.out_dir) {
        const char* names[3] = {"disp.f32", "occ.f32", "conf.f32"};
        for (int k = 0; k < 3; ++k)
            if (download_and_write(dout[k].h, map * sizeof(float), std::string(o.out_dir) + "/" + names[k], "cannot write the outputs")) return 1;
    }
    if (o.repeat > 0) {
        for (int i = 0; i < 3; ++i)                                  // warm-up: the second run captures the graph
            if (forward()) return 1;
        HIP_OK(hipStreamSynchronize(c.s), "warm-up");
        float ms = 0.f;
        if (time_calls(c.s, o.repeat, forward, &ms, "timed runs")) return 1;
        printf("{\"B\": %d, \"H\": %d, \"W\": %d, \"repeat\": %d, \"ms_per_pair\": %.4f}\n", m.B, m.H, m.W, o.repeat, ms / o.repeat / m.B);
    }
    const bool cloud = o.calib_path && (o.ply_path || o.mesh_path);
    if (o.min_size_arg || cloud || o.register_cam || o.voxel_arg || o.normals_path || o.smooth_arg) {   // the calibration: once, in front of the first 3D stage
        if (!read_calib(o.calib_path, c.cal)) return fail("--calib: cannot read cam0 and baseline from the file");
        if (m.out_h != m.H || m.out_w != m.W) return fail("the 3D outputs need maps of the image's size (an engine without output_upsample)");
    }
    if (o.min_size_arg && stage_segment(c)) return 1;
    if (o.smooth_arg && stage_smooth(c)) return 1;
    if (cloud && stage_cloud(c)) return 1;
    if (o.voxel_arg && stage_voxel(c)) return 1;
    if (o.register_cam && stage_register(c)) return 1;
    if (o.normals_path && stage_normals(c)) return 1;
    if (o.gt_path && stage_eval(c, g)) return 1;
    return 0;
}
