// Stand-alone host check of the runner's host side (s2m2_amd/app/runner_host.h): the option table and the rules between options on every row of
// tests/test_runner_cpu.py, the readers of everything the program is given from outside (PFM, calib, camera, thresholds) on good, damaged and
// hostile input, the names and the bytes of the files it leaves, the quantile and the JSON numbers -- as plain calls: host code only, no device,
// no library.  It writes its small inputs into a temporary directory of its own.  Meant for a sanitizer build, run from the repository root
// (or with the path of tests/golden/bicycle2_calib.txt as its argument):
//
//     hipcc --offload-host-only -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/runner_host_checks.cpp -o runner_host_checks
//     ./runner_host_checks        (prints "ok: N checks", exit status 0)
#include "../s2m2_amd/app/runner_host.h"

#include <unistd.h>

#include <utility>

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        ++g_checks;                                                   \
        if (!(cond)) {                                                \
            ++g_failed;                                               \
            fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
        }                                                             \
    } while (0)

static std::string g_dir;
static std::string in_dir(const char* name) { return g_dir + "/" + name; }

static void put(const char* name, const std::string& bytes) {
    FILE* f = fopen(in_dir(name).c_str(), "wb");
    if (!f || fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size() || fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", in_dir(name).c_str());
        exit(2);
    }
}

static std::string get(const char* name) {
    std::string s;
    FILE* f = fopen(in_dir(name).c_str(), "rb");
    for (int ch; f && (ch = fgetc(f)) != EOF;) s.push_back((char)ch);
    if (f) fclose(f);
    return s;
}

// a PFM of `values`, rows bottom to top as the format has them; big: every float32 byte-swapped
static std::string pfm(const char* head, const std::vector<float>& values, bool big = false) {
    std::string s = head;
    for (const float v : values) {
        char b[4];
        memcpy(b, &v, 4);
        if (big) { std::swap(b[0], b[3]); std::swap(b[1], b[2]); }
        s.append(b, 4);
    }
    return s;
}

// what the program says for this command line (ENGINE LEFT RIGHT in front): USAGE, a message, or "engine" where the options are complete
static std::string outcome(std::vector<std::string> args) {
    args.insert(args.begin(), {"s2m2_run_engine", "absent.s2m2", "l.f32", "r.f32"});
    std::vector<char*> argv;
    for (std::string& a : args) argv.push_back(&a[0]);
    Options o;
    if (!parse_options((int)argv.size(), argv.data(), o)) return USAGE;
    if (const char* msg = check_options(o)) return msg;
    GroundTruth g;
    const std::string msg = read_ground_truth(o, g);
    return msg.empty() ? "engine" : msg;
}
static bool says(const std::vector<std::string>& args, const char* want) { return outcome(args).find(want) != std::string::npos; }

static bool thresholds(const char* arg, std::vector<float> want) {
    float thr[S2M2_EVAL_MAX_THR];
    int n = -1;
    if (!parse_thresholds(arg, thr, n)) return false;
    return std::vector<float>(thr, thr + n) == want;
}
static bool thresholds_refused(const char* arg) {
    float thr[S2M2_EVAL_MAX_THR];
    int n = -1;
    return !parse_thresholds(arg, thr, n);
}

int main(int argc, char** argv) {
    char tmpl[] = "/tmp/runner_host_checks.XXXXXX";
    if (!mkdtemp(tmpl)) return 2;
    g_dir = tmpl;
    const char* golden_calib = argc > 1 ? argv[1] : "tests/golden/bicycle2_calib.txt";

    // ---- read_pfm: 3 x 2, file rows bottom to top -> memory rows top to bottom
    const std::vector<float> bottom_up = {4, 5, 6, 1, 2, 3}, top_down = {1, 2, 3, 4, 5, 6};
    const char *NOT_PFM = "not a greyscale PFM (header Pf, width height, scale)", *NOT_DATA = "the data is not width * height float32 values";
    std::vector<float> v;
    int w = 0, h = 0;
    const char* why = "";
    put("le.pfm", pfm("Pf\n3 2\n-1.0\n", bottom_up));
    CHECK(read_pfm(in_dir("le.pfm").c_str(), v, w, h, why) && w == 3 && h == 2 && v == top_down);
    put("be.pfm", pfm("Pf\n3 2\n1.0\n", bottom_up, true));
    v.clear();
    CHECK(read_pfm(in_dir("be.pfm").c_str(), v, w, h, why) && w == 3 && h == 2 && v == top_down);
    const auto refused = [&](const char* name, const char* want) {
        std::vector<float> x;
        int ww = 0, hh = 0;
        const char* y = "";
        return !read_pfm(in_dir(name).c_str(), x, ww, hh, y) && strcmp(y, want) == 0;
    };
    put("short.pfm", pfm("Pf\n3 2\n-1.0\n", {4, 5, 6, 1, 2}));
    CHECK(refused("short.pfm", NOT_DATA));
    put("long.pfm", pfm("Pf\n3 2\n-1.0\n", {4, 5, 6, 1, 2, 3, 7}));
    CHECK(refused("long.pfm", NOT_DATA));
    put("colour.pfm", pfm("PF\n3 2\n-1.0\n", bottom_up));
    CHECK(refused("colour.pfm", NOT_PFM));
    put("scale0.pfm", pfm("Pf\n3 2\n0\n", bottom_up));
    CHECK(refused("scale0.pfm", NOT_PFM));
    put("width0.pfm", pfm("Pf\n0 2\n-1.0\n", bottom_up));
    CHECK(refused("width0.pfm", NOT_PFM));
    put("huge.pfm", pfm("Pf\n65536 32768\n-1.0\n", bottom_up));          // width * height = 2^31: refused before anything is allocated
    CHECK(refused("huge.pfm", NOT_PFM));
    CHECK(refused("absent.pfm", "cannot open the file"));

    // ---- read_calib
    Calib cal;
    CHECK(read_calib(golden_calib, cal));
    CHECK(cal.fx == 3896.34 && cal.cx == 1064.836 && cal.cy == 976.456 && cal.doffs == 163.863 && cal.baseline == 173.557 && cal.have_cam1);
    put("nobase.txt", "cam0=[1000 0 320; 0 1000 240; 0 0 1]\ndoffs=0\n");
    Calib nobase;
    CHECK(!read_calib(in_dir("nobase.txt").c_str(), nobase) && nobase.have_cam0 && !nobase.have_baseline);
    put("longline.txt", "note=" + std::string(2000, 'x') + "\ncam0=[1000 0 320; 0 1001 240; 0 0 1]\nbaseline=100\n");   // four reads of the 512-byte buffer
    Calib longline;
    CHECK(read_calib(in_dir("longline.txt").c_str(), longline) && longline.fx == 1000 && longline.fy == 1001 && longline.baseline == 100);
    Calib absent;
    CHECK(!read_calib(in_dir("absent.txt").c_str(), absent));

    // ---- read_camera
    TargetCamera cam;
    put("cam_min.txt", "width=640\nheight=480\ncam=[500 0 320; 0 501 240; 0 0 1]\n");
    CHECK(read_camera(in_dir("cam_min.txt").c_str(), cam) && cam.width == 640 && cam.height == 480 && cam.fx == 500 && cam.fy == 501 &&
          cam.cx == 320 && cam.cy == 240);
    const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero[3] = {0, 0, 0};
    CHECK(memcmp(cam.R, eye, sizeof eye) == 0 && memcmp(cam.t, zero, sizeof zero) == 0);
    TargetCamera full;
    put("cam_full.txt", "width=64\nheight=48\ncam=[50 0 32; 0 51 24; 0 0 1]\nR=[0 -1 0; 1 0 0; 0 0 1]\nt=[0.1 -0.2 0.3]\n");
    const double rot[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, tr[3] = {0.1, -0.2, 0.3};
    CHECK(read_camera(in_dir("cam_full.txt").c_str(), full) && full.width == 64 && full.height == 48 && full.fx == 50 && full.cy == 24);
    CHECK(memcmp(full.R, rot, sizeof rot) == 0 && memcmp(full.t, tr, sizeof tr) == 0);
    const auto camera_refused = [&](const char* name) {
        TargetCamera fresh;
        return !read_camera(in_dir(name).c_str(), fresh);
    };
    put("cam_nocam.txt", "width=640\nheight=480\n");
    CHECK(camera_refused("cam_nocam.txt"));
    put("cam_nowidth.txt", "height=480\ncam=[500 0 320; 0 501 240; 0 0 1]\n");
    CHECK(camera_refused("cam_nowidth.txt"));
    put("cam_width0.txt", "width=0\nheight=480\ncam=[500 0 320; 0 501 240; 0 0 1]\n");
    CHECK(camera_refused("cam_width0.txt"));
    put("cam_widthneg.txt", "width=-640\nheight=480\ncam=[500 0 320; 0 501 240; 0 0 1]\n");
    CHECK(camera_refused("cam_widthneg.txt"));

    // ---- the threshold list
    CHECK(thresholds("0.5,1,2,4", {0.5f, 1.f, 2.f, 4.f}) && thresholds("1,2,3,4,5,6,7,8", {1, 2, 3, 4, 5, 6, 7, 8}));
    CHECK(thresholds("1,2,", {1.f, 2.f}));
    CHECK(thresholds("", {}));
    CHECK(thresholds_refused("1,1") && thresholds_refused("2,1") && thresholds_refused("0") && thresholds_refused("-1"));
    CHECK(thresholds_refused("1,2,3,4,5,6,7,8,9"));
    CHECK(thresholds_refused("0.5;1") && thresholds_refused("x") && thresholds_refused(",1") && thresholds_refused("inf") && thresholds_refused("nan"));

    // ---- pair_path
    CHECK(pair_path("OUT.ply", 1, 0) == "OUT.ply" && pair_path("OUT", 1, 0) == "OUT");
    CHECK(pair_path("OUT.ply", 2, 1) == "OUT.1.ply" && pair_path("OUT", 2, 1) == "OUT.1.ply");
    CHECK(pair_path("a.f32", 2, 0, ".f32") == "a.0.f32" && pair_path("a.ply", 2, 0, ".f32") == "a.ply.0.f32");
    CHECK(pair_path(".ply", 2, 1) == ".ply.1.ply");                  // a stem that is the extension alone keeps it

    // ---- eval_quantile (bins of 1/64 px, the last one the overflow bin)
    std::vector<unsigned long long> hist(S2M2_EVAL_HIST_BINS, 0);
    CHECK(isnan(eval_quantile(hist.data(), 0.5)));
    hist[0] = 7;
    CHECK(eval_quantile(hist.data(), 0.5) == 1.0 / 64 && eval_quantile(hist.data(), 0.99) == 1.0 / 64 && eval_quantile(hist.data(), 0.0) == 1.0 / 64);
    hist[0] = 0;
    hist[S2M2_EVAL_HIST_BINS - 1] = 3;
    CHECK(isinf(eval_quantile(hist.data(), 0.5)) && isinf(eval_quantile(hist.data(), 0.01)));
    hist[S2M2_EVAL_HIST_BINS - 1] = 0;
    hist[0] = 1;                                                     // 1 of 4 in bin 0, 3 of 4 in bin 3: the quarter is reached in bin 0
    hist[3] = 3;
    CHECK(eval_quantile(hist.data(), 0.25) == 1.0 / 64 && eval_quantile(hist.data(), 0.26) == 4.0 / 64 && eval_quantile(hist.data(), 0.99) == 4.0 / 64);

    // ---- json_number
    {
        FILE* f = fopen(in_dir("n.json").c_str(), "w");
        if (!f) return 2;
        json_number(f, "a", NAN, ", ");
        json_number(f, "b", INFINITY, ", ");
        json_number(f, "c", -INFINITY, ", ");
        json_number(f, "d", 0.25, "");
        fclose(f);
        CHECK(get("n.json") == "\"a\": null, \"b\": null, \"c\": null, \"d\": 0.25");
    }

    // ---- the files: write_bytes, write_ply, write_ply_mesh
    unsigned char rec[32];
    for (int i = 0; i < 32; ++i) rec[i] = (unsigned char)(i + 1);
    const int32_t face[3] = {0, 1, 0};
    const std::string vertex_head = "ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
                                    "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n";
    const std::string rec_bytes((const char*)rec, 32);
    CHECK(write_ply(in_dir("c.ply"), rec, 2) && get("c.ply") == vertex_head + "end_header\n" + rec_bytes);
    CHECK(write_ply_mesh(in_dir("m.ply"), rec, 2, face, 1));
    const std::string mesh_head = vertex_head + "element face 1\nproperty list uchar int vertex_indices\nend_header\n", mesh = get("m.ply");
    CHECK(mesh.size() == mesh_head.size() + 2 * 16 + 13 && mesh.compare(0, mesh_head.size(), mesh_head) == 0);
    CHECK(mesh.size() > mesh_head.size() + 32 && mesh[mesh_head.size() + 32] == 3 && memcmp(mesh.data() + mesh_head.size() + 33, face, 12) == 0 &&
          mesh.compare(mesh_head.size(), 32, rec_bytes) == 0);
    CHECK(write_ply_mesh(in_dir("m0.ply"), rec, 0, face, 0) && get("m0.ply").find("element vertex 0\n") != std::string::npos);
    CHECK(write_bytes(in_dir("p.ppm"), "P6\n1 1\n255\n", rec, 3) && get("p.ppm") == std::string("P6\n1 1\n255\n\x01\x02\x03"));
    CHECK(!write_bytes(in_dir("no_such_dir/x"), "", rec, 3) && !write_ply(in_dir("no_such_dir/x"), rec, 2));
    std::vector<unsigned char> six(6), five(5);
    put("r6.u8", std::string(6, '\x01'));
    CHECK(read_raw_u8(in_dir("r6.u8").c_str(), six) && six[5] == 1 && !read_raw_u8(in_dir("r6.u8").c_str(), five) && !read_raw_u8(in_dir("absent.u8").c_str(), six));
    std::vector<float> six_f(6), one_f(1);
    CHECK(read_raw(in_dir("le.pfm").c_str(), one_f) == false && !read_raw(in_dir("r6.u8").c_str(), six_f));
    put("one.f32", pfm("", {2.5f}));
    CHECK(read_raw(in_dir("one.f32").c_str(), one_f) && one_f[0] == 2.5f);

    // ---- fill_cloud_inputs: every input field, no output field
    {
        s2m2_engine_info m;
        memset(&m, 0, sizeof m);
        m.B = 2; m.H = 30; m.W = 50; m.out_h = 32; m.out_w = 64;
        Options o;
        o.depth_scale = 100.0; o.depth_trunc = 3.0; o.conf_min = 0.2; o.occ_min = 0.6;
        s2m2_cloud_desc cd;
        memset(&cd, 0, sizeof cd);
        const float maps[3] = {0, 0, 0};
        fill_cloud_inputs(cd, m, maps, maps + 1, maps + 2, rec, 2, 1, cal, o);
        CHECK(cd.disp == maps && cd.occ == maps + 1 && cd.conf == maps + 2 && cd.image == rec && cd.image_dtype == 2 && cd.unfiltered == 1);
        CHECK(cd.B == 2 && cd.H == 30 && cd.W == 50 && cd.Hp == 32 && cd.Wp == 64);
        CHECK(cd.fx == cal.fx && cd.fy == cal.fy && cd.cx == cal.cx && cd.cy == cal.cy && cd.baseline == cal.baseline && cd.doffs == cal.doffs);
        CHECK(cd.depth_scale == 100.0 && cd.depth_trunc == 3.0 && cd.conf_min == 0.2 && cd.occ_min == 0.6);
        CHECK(!cd.depth && !cd.mask && !cd.records && !cd.count && !cd.workspace && cd.capacity == 0);
    }

    // ---- the command line: every row of tests/test_runner_cpu.py
    const std::string C = golden_calib;
    const std::vector<std::string> REG = {"--calib", C, "--register", "right", "--register-depth", "x.f32"};
    const auto reg = [&](std::vector<std::string> more) {
        more.insert(more.begin(), REG.begin(), REG.end());
        return more;
    };
    CHECK(says({}, "engine"));
    CHECK(says({"--bogus"}, "usage: s2m2_run_engine ENGINE LEFT RIGHT") && says({"fourth"}, "usage: ") && says({"--repeat", "-1"}, "usage: ") && says({"--out"}, "usage: "));
    CHECK(says({"--ply", "x.ply"}, "--calib and --ply come together") && says({"--calib", C}, "--calib and --ply come together"));
    CHECK(says({"--calib", C, "--depth", "d.f32"}, "--calib and --ply come together"));
    CHECK(says({"--calib", C, "--ply", "x.ply"}, "engine"));
    CHECK(says({"--mesh", "x.ply"}, "--calib and --mesh come together") && says({"--calib", C, "--mesh", "x.ply"}, "engine"));
    CHECK(says({"--calib", C, "--mesh", "x.ply", "--max-jump", "inf"}, "engine"));
    for (const char* x : {"-1", "nan", "1x"}) CHECK(says({"--calib", C, "--mesh", "x.ply", "--max-jump", x}, "--max-jump: a number >= 0 (inf is allowed)"));
    CHECK(says({"--calib", C, "--ply", "x.ply", "--max-jump", "1"}, "--max-jump needs --mesh or --min-size"));
    CHECK(says({"--image", "i.u8"}, "--image and --depth need --calib and --ply") && says({"--depth", "d.f32"}, "--image and --depth need --calib and --ply"));
    CHECK(says(reg({"--depth", "d.f32"}), "--depth needs --ply or --mesh"));
    CHECK(says({"--calib", C, "--min-size", "5", "--depth", "d.f32"}, "--depth needs --ply or --mesh") && says({"--calib", C, "--min-size", "5"}, "engine"));
    CHECK(says({"--register", "right", "--register-depth", "x.f32"}, "--register needs --calib and --register-depth"));
    CHECK(says({"--calib", C, "--register", "right"}, "--register needs --calib and --register-depth"));
    CHECK(says({"--calib", C, "--ply", "x.ply", "--splat", "2"}, "--splat and --register-* need --register"));
    CHECK(says({"--calib", C, "--ply", "x.ply", "--register-image", "x.ppm"}, "--splat and --register-* need --register"));
    CHECK(says(reg({"--splat", "5"}), "--splat: 1, 2, 3 or 4") && says(reg({"--splat", "0"}), "--splat: 1, 2, 3 or 4") && says(reg({}), "engine"));
    CHECK(says({"--min-size", "5"}, "--min-size needs --calib"));
    for (const char* x : {"0", "five", "1073741825"}) CHECK(says({"--calib", C, "--min-size", x}, "--min-size: an integer >= 1 (at most 2^30)"));
    CHECK(says({"--calib", C, "--ply", "x.ply", "--labels", "x.i32"}, "--labels and --segment-mask need --min-size"));
    CHECK(says({"--calib", C, "--ply", "x.ply", "--segment-mask", "x.u8"}, "--labels and --segment-mask need --min-size"));
    CHECK(says({"--gt", "ok.pfm"}, "--gt and --metrics come together") && says({"--metrics", "m.json"}, "--gt and --metrics come together"));
    CHECK(says({"--gt-region", "r.u8"}, "--gt-region and --thresholds need --gt and --metrics"));
    CHECK(says({"--thresholds", "1,2"}, "--gt-region and --thresholds need --gt and --metrics"));
    put("r5.u8", std::string(5, '\x01'));
    const auto gt = [&](const char* file, std::vector<std::string> more) {
        more.insert(more.begin(), {"--gt", in_dir(file), "--metrics", "m.json"});
        return more;
    };
    CHECK(says(gt("le.pfm", {}), "engine") && says(gt("le.pfm", {"--gt-min", "-inf"}), "engine") && says(gt("le.pfm", {"--thresholds", "1,2,"}), "engine"));
    CHECK(says(gt("le.pfm", {"--gt-region", in_dir("r6.u8")}), "engine"));
    CHECK(outcome(gt("absent.pfm", {})) == "--gt " + in_dir("absent.pfm") + ": cannot open the file");
    CHECK(says(gt("short.pfm", {}), NOT_DATA) && says(gt("long.pfm", {}), NOT_DATA) && says(gt("colour.pfm", {}), NOT_PFM) && says(gt("scale0.pfm", {}), NOT_PFM));
    CHECK(says(gt("le.pfm", {"--gt-region", in_dir("r5.u8")}), "--gt-region must be a raw uint8 file of the ground truth's 3 x 2 pixels"));
    for (const char* x : {"1,1", "1,2,3,4,5,6,7,8,9", "0.5;1"})
        CHECK(says(gt("le.pfm", {"--thresholds", x}), "--thresholds: up to 8 numbers > 0, strictly increasing, separated by commas"));
    CHECK(says(gt("le.pfm", {"--gt-min", "nan"}), "--gt-min: not a number"));
    // the numbers behind the messages: defaults, the last of a repeated option, the flag
    {
        std::vector<std::string> a = {"x", "e", "l", "r", "--calib", C, "--min-size", "7", "--max-jump", "inf", "--unfiltered", "--repeat", "3", "--repeat", "4",
                                      "--conf-min", "0.02", "--depth-trunc", "abc"};
        std::vector<char*> av;
        for (std::string& s : a) av.push_back(&s[0]);
        Options o;
        CHECK(parse_options((int)av.size(), av.data(), o) && check_options(o) == nullptr);
        CHECK(o.npos == 3 && o.repeat == 4 && o.min_size == 7 && isinf(o.max_jump) && o.unfiltered == 1 && o.conf_min == 0.02 && o.depth_trunc == 0.0);
        CHECK(o.splat == 2 && o.depth_scale == 1000.0 && o.occ_min == 0.5 && o.gt_min == 0.0 && !o.ply_path && !o.gt_path);
    }

    // ---- --tsdf-frames (K24): the mode's rules, the numbers it parses, and LIST
    {
        const auto tsdf = [&](std::vector<std::string> args, Options& o) -> std::string {
            args.insert(args.begin(), {"s2m2_run_engine", "absent.s2m2"});
            std::vector<char*> av;
            for (std::string& s : args) av.push_back(&s[0]);
            if (!parse_options((int)av.size(), av.data(), o)) return USAGE;
            const char* msg = check_options(o);
            return msg ? msg : "engine";
        };
        const std::vector<std::string> full = {"--tsdf-frames", "l.txt", "--tsdf-dims", "19,13,11", "--tsdf-voxel", "0.1", "--tsdf-origin", "-0.9,-0.6,1.5",
                                               "--calib", golden_calib, "--tsdf-ply", "t.ply"};
        Options o;
        CHECK(tsdf(full, o) == "engine");
        CHECK(o.tsdf_dims[0] == 19 && o.tsdf_dims[1] == 13 && o.tsdf_dims[2] == 11 && o.tsdf_voxel == 0.1 && o.tsdf_trunc == 0.4 && o.tsdf_min_weight == 1);
        CHECK(o.tsdf_origin[0] == -0.9 && o.tsdf_origin[1] == -0.6 && o.tsdf_origin[2] == 1.5 && !o.tsdf_carve);
        std::vector<std::string> more = full;
        more.insert(more.end(), {"--tsdf-trunc", "0.25", "--tsdf-min-weight", "3", "--tsdf-carve"});
        Options o2;
        CHECK(tsdf(more, o2) == "engine" && o2.tsdf_trunc == 0.25 && o2.tsdf_min_weight == 3 && o2.tsdf_carve == 1);
        const auto with = [&](const char* flag, const char* value) {
            std::vector<std::string> a = full;
            for (size_t i = 0; i + 1 < a.size(); ++i)
                if (a[i] == flag) a[i + 1] = value;
            Options x;
            return tsdf(a, x);
        };
        for (const char* bad : {"19,13", "19,13,11,2", "19,13,0", "1.5,2,3", "1024,1024,512", "", ",,", "19,13,11x"})
            CHECK(with("--tsdf-dims", bad).find("--tsdf-dims: three integers") == 0);
        for (const char* bad : {"0", "-1", "nan", "inf", "1e400", "", "5cm"}) CHECK(with("--tsdf-voxel", bad) == "--tsdf-voxel: a number > 0");
        for (const char* bad : {"0,0", "0,0,nan", "0,0,inf", "a,b,c", "0,0,0,0"}) CHECK(with("--tsdf-origin", bad).find("--tsdf-origin: three finite numbers") == 0);
        Options o3;
        CHECK(tsdf({"--tsdf-dims", "1,1,1"}, o3).find("need --tsdf-frames") != std::string::npos);
        Options o4;
        std::vector<std::string> pair = full;
        pair.insert(pair.begin(), {"l.f32", "r.f32"});
        CHECK(tsdf(pair, o4).find("takes ENGINE alone") != std::string::npos);
        // --tsdf-mesh (K25): an option of the mode, with the size limit of an int32 face count
        std::vector<std::string> meshed = full;
        meshed.insert(meshed.end(), {"--tsdf-mesh", "m.ply"});
        Options o5, o6, o7;
        CHECK(tsdf(meshed, o5) == "engine" && std::string(o5.tsdf_mesh_path) == "m.ply" && o.tsdf_mesh_path == nullptr);
        CHECK(tsdf({"--tsdf-mesh", "m.ply"}, o6).find("need --tsdf-frames") != std::string::npos);
        for (size_t i = 0; i + 1 < meshed.size(); ++i)
            if (meshed[i] == "--tsdf-dims") meshed[i + 1] = "1024,1024,410";
        CHECK(tsdf(meshed, o7).find("--tsdf-mesh: NX*NY*NZ <= 429496729") == 0);
        CHECK(with("--tsdf-dims", "1024,1024,410") == "engine");
        // --tsdf-render (K26): the pose, one of the two maps at least, the step and the weight with their defaults
        const char* pose = "1,0,0,0.5,0,1,0,-0.25,0,0,1,2";
        const auto rendered = [&](std::vector<std::string> extra, Options& x) {
            std::vector<std::string> a = full;
            a.insert(a.end(), {"--tsdf-trunc", "0.25", "--tsdf-min-weight", "3"});
            a.insert(a.end(), extra.begin(), extra.end());
            return tsdf(a, x);
        };
        Options r0, r1, r2, r3;
        CHECK(rendered({"--tsdf-render", pose, "--tsdf-render-depth", "d.f32"}, r0) == "engine");
        CHECK(r0.tsdf_render_pose[0] == 1.f && r0.tsdf_render_pose[3] == 0.5f && r0.tsdf_render_pose[7] == -0.25f && r0.tsdf_render_pose[11] == 2.f);
        CHECK(r0.tsdf_render_step == 0.125 && r0.tsdf_render_min_weight == 3 && r0.tsdf_render_image_path == nullptr);
        CHECK(rendered({"--tsdf-render", pose, "--tsdf-render-image", "i.u8", "--tsdf-render-step", "0.05", "--tsdf-render-min-weight", "1"}, r1) == "engine");
        CHECK(r1.tsdf_render_step == 0.05 && r1.tsdf_render_min_weight == 1 && r1.tsdf_render_image_path != nullptr && r1.tsdf_render_depth_path == nullptr);
        CHECK(rendered({"--tsdf-render", pose}, r2) == "--tsdf-render needs --tsdf-render-depth or --tsdf-render-image");
        for (const char* flag : {"--tsdf-render-depth", "--tsdf-render-image", "--tsdf-render-step", "--tsdf-render-min-weight"}) {
            Options x;
            CHECK(rendered({flag, "1"}, x) == "the --tsdf-render-* options need --tsdf-render");
        }
        CHECK(tsdf({"--tsdf-render", pose, "--tsdf-render-depth", "d.f32"}, r3).find("need --tsdf-frames") != std::string::npos);
        for (const char* bad : {"1,0,0,0,0,1,0,0,0,0,1", "1,0,0,0,0,1,0,0,0,0,1,0,0", "1,0,0,0,0,1,0,0,0,0,1,nan", "1,0,0,0,0,1,0,0,0,0,1,inf", "", "1 0 0 0 0 1 0 0 0 0 1 0",
                                "1,0,0,0,0,1,0,0,0,0,1,1e39", "1,0,0,0,0,1,0,0,0,0,1,0x"}) {
            Options x;
            CHECK(rendered({"--tsdf-render", bad, "--tsdf-render-depth", "d.f32"}, x).find("--tsdf-render: twelve finite numbers") == 0);
        }
        for (const char* bad : {"0", "-1", "nan", "inf", "", "1mm"}) {
            Options x;
            CHECK(rendered({"--tsdf-render", pose, "--tsdf-render-depth", "d.f32", "--tsdf-render-step", bad}, x) == "--tsdf-render-step: a number > 0");
        }
        for (const char* bad : {"0", "-1", "32768", "two", "1.5", ""}) {
            Options x;
            CHECK(rendered({"--tsdf-render", pose, "--tsdf-render-depth", "d.f32", "--tsdf-render-min-weight", bad}, x) == "--tsdf-render-min-weight: an integer in 1..32767");
        }
        // --tsdf-track (K27): the flag, the iterations and the gate with their defaults
        Options k0, k1, k2;
        CHECK(rendered({"--tsdf-track"}, k0) == "engine" && k0.tsdf_track == 1 && k0.tsdf_track_iters == 10 && k0.tsdf_track_dist == 0.25 && !k0.tsdf_poses_out_path);
        CHECK(rendered({"--tsdf-track", "--tsdf-track-iters", "64", "--tsdf-track-dist", "0.5", "--tsdf-poses-out", "p.txt"}, k1) == "engine");
        CHECK(k1.tsdf_track_iters == 64 && k1.tsdf_track_dist == 0.5 && k1.tsdf_poses_out_path != nullptr && r0.tsdf_track == 0);
        CHECK(tsdf({"--tsdf-track"}, k2).find("need --tsdf-frames") != std::string::npos);
        for (const char* flag : {"--tsdf-track-iters", "--tsdf-track-dist", "--tsdf-poses-out"}) {
            Options x;
            CHECK(rendered({flag, "1"}, x) == "--tsdf-track-iters, --tsdf-track-dist and --tsdf-poses-out need --tsdf-track");
        }
        for (const char* bad : {"0", "-1", "65", "ten", "2.5", ""}) {
            Options x;
            CHECK(rendered({"--tsdf-track", "--tsdf-track-iters", bad}, x) == "--tsdf-track-iters: an integer in 1..64");
        }
        for (const char* bad : {"0", "-1", "nan", "inf", "", "2cm"}) {
            Options x;
            CHECK(rendered({"--tsdf-track", "--tsdf-track-dist", bad}, x) == "--tsdf-track-dist: a number > 0");
        }
        {
            const float at[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};                       // the camera in the world's origin
            const float back[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1};                     // p_cam = p + (0,0,1): the centre is (0,0,-1)
            const int dims[3] = {3, 5, 9};
            const double origin[3] = {-1.0, -2.0, 1.0};
            CHECK(tsdf_far_corner(at, dims, origin, 0.5) == sqrt(1.0 + 4.0 + 25.0));         // corners x -1 | 0, y -2 | 0, z 1 | 5
            CHECK(tsdf_far_corner(back, dims, origin, 0.5) == sqrt(1.0 + 4.0 + 36.0));
        }

        std::vector<TsdfFrame> fr;
        put("frames.txt", "# head\n\nl0.f32 r0.f32 i0.u8 1 0 0 0.5 0 1 0 -0.25 0 0 1 2\n   l1.f32 r1.f32 i1.u8 1 0 0 0 0 1 0 0 0 0 1 0   \n");
        CHECK(read_tsdf_frames(in_dir("frames.txt").c_str(), fr).empty() && fr.size() == 2);
        CHECK(fr.size() == 2 && fr[0].left == "l0.f32" && fr[0].image == "i0.u8" && fr[0].pose[3] == 0.5f && fr[0].pose[7] == -0.25f && fr[0].pose[11] == 2.f &&
              fr[1].right == "r1.f32");
        const auto list_says = [&](const std::string& text, const char* want) {
            std::vector<TsdfFrame> x;
            put("frames.txt", text);
            return read_tsdf_frames(in_dir("frames.txt").c_str(), x).find(want) != std::string::npos;
        };
        CHECK(list_says("", "no frame") && list_says("# only\n", "no frame"));
        CHECK(list_says("l r i 1 0 0 0 0 1 0 0 0 0 1\n", "line 1: "));                       // eleven numbers
        CHECK(list_says("l r i 1 0 0 0 0 1 0 0 0 0 1 0 9\n", "line 1: "));                   // thirteen
        CHECK(list_says("l r 1 0 0 0 0 1 0 0 0 0 1 0\n", "line 1: "));                       // two names
        CHECK(list_says("l r i 1 0 0 0 0 1 0 0 0 0 1 0\nl r i 1 0 0 inf 0 1 0 0 0 0 1 0\n", "line 2: "));
        CHECK(list_says(std::string(5000, 'x') + " r i 1 0 0 0 0 1 0 0 0 0 1 0\n", "line 1: "));     // a name longer than the line buffer
        std::vector<TsdfFrame> none;
        CHECK(read_tsdf_frames(in_dir("absent.txt").c_str(), none).find("cannot open") != std::string::npos);
        unlink(in_dir("frames.txt").c_str());
    }

    for (const char* name : {"le.pfm", "be.pfm", "short.pfm", "long.pfm", "colour.pfm", "scale0.pfm", "width0.pfm", "huge.pfm", "nobase.txt", "longline.txt",
                             "cam_min.txt", "cam_full.txt", "cam_nocam.txt", "cam_nowidth.txt", "cam_width0.txt", "cam_widthneg.txt", "n.json", "c.ply", "m.ply",
                             "m0.ply", "p.ppm", "r6.u8", "r5.u8", "one.f32"})
        unlink(in_dir(name).c_str());
    rmdir(g_dir.c_str());
    if (g_failed) {
        fprintf(stderr, "%d of %d checks failed\n", g_failed, g_checks);
        return 1;
    }
    printf("ok: %d checks\n", g_checks);
    return 0;
}
