"""The runner's command line without a GPU (s2m2_amd/app/run_engine.cpp, runner_host.h): every rule between options, every numeric option that
can be refused and the ground-truth files, which are all decided before the engine is loaded.  The texts were recorded from the runner before
its host side moved into runner_host.h: they are the pin.  An engine file that does not exist is the last failure a complete command line can
reach here."""
import os
import struct
import subprocess

import pytest

from s2m2_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = os.path.join(ROOT, "tests", "golden", "bicycle2_calib.txt")
ENGINE = "cannot load the engine: engine_load: cannot open absent.s2m2"
USAGE = "usage: s2m2_run_engine ENGINE LEFT RIGHT"
REG = ["--calib", C, "--register", "right", "--register-depth", "x.f32"]
MAX_JUMP = "--max-jump: a number >= 0 (inf is allowed)"
MIN_SIZE = "--min-size: an integer >= 1 (at most 2^30)"
THRESHOLDS = "--thresholds: up to 8 numbers > 0, strictly increasing, separated by commas"
NOT_PFM = "not a greyscale PFM (header Pf, width height, scale)"
NOT_DATA = "the data is not width * height float32 values"

# (options, what stderr contains)
OPTION_ROWS = [
    ([], ENGINE),
    (["--bogus"], USAGE),
    (["fourth"], USAGE),
    (["--repeat", "-1"], USAGE),
    (["--out"], USAGE),
    (["--ply", "x.ply"], "--calib and --ply come together"),
    (["--calib", C], "--calib and --ply come together"),
    (["--calib", C, "--depth", "d.f32"], "--calib and --ply come together"),
    (["--calib", C, "--ply", "x.ply"], ENGINE),
    (["--mesh", "x.ply"], "--calib and --mesh come together"),
    (["--calib", C, "--mesh", "x.ply"], ENGINE),
    (["--calib", C, "--mesh", "x.ply", "--max-jump", "inf"], ENGINE),
    (["--calib", C, "--mesh", "x.ply", "--max-jump", "-1"], MAX_JUMP),
    (["--calib", C, "--mesh", "x.ply", "--max-jump", "nan"], MAX_JUMP),
    (["--calib", C, "--mesh", "x.ply", "--max-jump", "1x"], MAX_JUMP),
    (["--calib", C, "--ply", "x.ply", "--max-jump", "1"], "--max-jump needs --mesh or --min-size"),
    (["--image", "i.u8"], "--image and --depth need --calib and --ply"),
    (["--depth", "d.f32"], "--image and --depth need --calib and --ply"),
    (REG + ["--depth", "d.f32"], "--depth needs --ply or --mesh"),
    (["--calib", C, "--min-size", "5", "--depth", "d.f32"], "--depth needs --ply or --mesh"),
    (["--calib", C, "--min-size", "5"], ENGINE),
    (["--register", "right", "--register-depth", "x.f32"], "--register needs --calib and --register-depth"),
    (["--calib", C, "--register", "right"], "--register needs --calib and --register-depth"),
    (["--calib", C, "--ply", "x.ply", "--splat", "2"], "--splat and --register-* need --register"),
    (["--calib", C, "--ply", "x.ply", "--register-image", "x.ppm"], "--splat and --register-* need --register"),
    (REG + ["--splat", "5"], "--splat: 1, 2, 3 or 4"),
    (REG + ["--splat", "0"], "--splat: 1, 2, 3 or 4"),
    (REG, ENGINE),
    (["--min-size", "5"], "--min-size needs --calib"),
    (["--calib", C, "--min-size", "0"], MIN_SIZE),
    (["--calib", C, "--min-size", "five"], MIN_SIZE),
    (["--calib", C, "--min-size", "1073741825"], MIN_SIZE),
    (["--calib", C, "--ply", "x.ply", "--labels", "x.i32"], "--labels and --segment-mask need --min-size"),
    (["--calib", C, "--ply", "x.ply", "--segment-mask", "x.u8"], "--labels and --segment-mask need --min-size"),
    (["--gt", "ok.pfm"], "--gt and --metrics come together"),
    (["--metrics", "m.json"], "--gt and --metrics come together"),
    (["--gt-region", "r.u8"], "--gt-region and --thresholds need --gt and --metrics"),
    (["--thresholds", "1,2"], "--gt-region and --thresholds need --gt and --metrics"),
]

# (the --gt file, further options, what stderr contains); the files are written by the `gt_dir` fixture
GT_ROWS = [
    ("ok.pfm", [], ENGINE),
    ("ok.pfm", ["--gt-min", "-inf"], ENGINE),
    ("ok.pfm", ["--thresholds", "1,2,"], ENGINE),
    ("ok.pfm", ["--gt-region", "r6.u8"], ENGINE),
    ("absent.pfm", [], "--gt absent.pfm: cannot open the file"),
    ("five.pfm", [], NOT_DATA),
    ("seven.pfm", [], NOT_DATA),
    ("colour.pfm", [], NOT_PFM),
    ("scale0.pfm", [], NOT_PFM),
    ("ok.pfm", ["--gt-region", "r5.u8"], "--gt-region must be a raw uint8 file of the ground truth's 3 x 2 pixels"),
    ("ok.pfm", ["--thresholds", "1,1"], THRESHOLDS),
    ("ok.pfm", ["--thresholds", "1,2,3,4,5,6,7,8,9"], THRESHOLDS),
    ("ok.pfm", ["--thresholds", "0.5;1"], THRESHOLDS),
    ("ok.pfm", ["--gt-min", "nan"], "--gt-min: not a number"),
]


@pytest.fixture(scope="module")
def lib():
    from s2m2_amd.build import build
    build(verbose=False)
    return hip.load()


@pytest.fixture(scope="module")
def gt_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("runner_gt")

    def pfm(name, head, nfloat):
        (d / name).write_bytes(head + struct.pack("<%df" % nfloat, *range(1, nfloat + 1)))

    pfm("ok.pfm", b"Pf\n3 2\n-1.0\n", 6)
    pfm("five.pfm", b"Pf\n3 2\n-1.0\n", 5)
    pfm("seven.pfm", b"Pf\n3 2\n-1.0\n", 7)
    pfm("colour.pfm", b"PF\n3 2\n-1.0\n", 6)
    pfm("scale0.pfm", b"Pf\n3 2\n0\n", 6)
    (d / "r6.u8").write_bytes(bytes(6))
    (d / "r5.u8").write_bytes(bytes(5))
    return d


def _run(extra, cwd=None):
    from s2m2_amd.build import RUNNER
    p = subprocess.run([RUNNER, "absent.s2m2", "l.f32", "r.f32"] + extra, capture_output=True, text=True, timeout=60, cwd=cwd)
    return p.returncode, p.stderr


@pytest.mark.parametrize("extra,msg", OPTION_ROWS, ids=lambda v: " ".join(os.path.basename(a) for a in v)[:60] if isinstance(v, list) else None)
def test_runner_options(lib, extra, msg):
    rc, err = _run(extra)
    assert rc == 1 and msg in err, (extra, rc, err)
    assert err.startswith("s2m2_run_engine: ") and err.count("\n") == 1


@pytest.mark.parametrize("gt,extra,msg", GT_ROWS, ids=lambda v: " ".join(v)[:40] if isinstance(v, list) else None)
def test_runner_ground_truth_files(lib, gt_dir, gt, extra, msg):
    rc, err = _run(["--gt", gt, "--metrics", "m.json"] + extra, cwd=gt_dir)          # (relative names: the messages quote them)
    assert rc == 1 and msg in err, (gt, extra, rc, err)
    assert err.startswith("s2m2_run_engine: ") and err.count("\n") == 1
    assert not (gt_dir / "m.json").exists()
