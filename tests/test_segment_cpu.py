"""CPU-side checks of K22 (include/s2m2_hip.h: s2m2_segment, s2m2_amd/cloud.py: segment): the boundary (symbols, descriptor layout, ABI version,
workspace and tile sizes, every validation path -- all of which return before any device call, there is no GPU here), the wrappers' own
errors, the runner's argument errors, and the numpy oracle the GPU tests compare against: on hand-computed 5x7 cases, against
scipy.ndimage.label where scipy exists, and against the face rule of mesh_oracle (a face never spans two components)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cloud_oracle
import mesh_oracle
import segment_oracle
from s2m2_amd import cloud, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(ROOT, "tests", "golden", "bicycle2_calib.txt")
F = np.float32
NAN, INF = float("nan"), float("inf")
# z = 100 / d metres: with depth_trunc 1000 a pixel is kept iff conf and occ pass and d > 0.1
CAM = dict(fx=1000.0, fy=1000.0, cx=3.0, cy=2.0, baseline=100.0, doffs=0.0, depth_trunc=1000.0)


@pytest.fixture(scope="module")
def lib():
    from s2m2_amd.build import build
    build(verbose=False)
    return hip.load()


def _desc(**over):
    """a descriptor that passes validation (the pointers are never dereferenced on the host); keys with a `cloud_` prefix go to the embedded
    s2m2_cloud_desc"""
    d = hip.SegmentDesc()
    c = d.cloud
    c.disp = c.occ = c.conf = 4096
    c.B, c.H, c.W, c.Hp, c.Wp, c.image_dtype = 1, 30, 50, 32, 64, 2
    c.fx, c.fy, c.cx, c.cy, c.baseline, c.doffs, c.depth_scale, c.depth_trunc, c.conf_min, c.occ_min = 1000.0, 1000.0, 25.0, 15.0, 100.0, 0.0, 1000.0, 3.0, 0.1, 0.5
    d.label = d.size = d.mask = d.stats = d.workspace = 8192
    d.disp_out = 16384
    d.max_jump, d.min_size = 1.0, 10
    for k, v in over.items():
        setattr(c if k.startswith("cloud_") else d, k[6:] if k.startswith("cloud_") else k, v)
    return d


def test_symbols_version_and_header_constant(lib):
    for name in ("s2m2_segment", "s2m2_segment_workspace_bytes", "s2m2_segment_tile_rows", "s2m2_segment_tile_cols"):
        assert hasattr(lib, name) and name in hip.SIGNATURES
    assert lib.s2m2_version() == 800 and hip.ABI_VERSION == 800
    header = open(os.path.join(ROOT, "include", "s2m2_hip.h")).read()
    assert int(re.search(r"#define S2M2_ABI_VERSION (\d+)", header).group(1)) == 800


def test_segment_desc_has_the_layout_of_the_header(tmp_path):
    """every field: offset and size of hip.SegmentDesc against s2m2_segment_desc compiled by gcc"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = [f[0] for f in hip.SegmentDesc._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "s2m2_hip.h"', "int main(void) {", "  s2m2_segment_desc d;",
             '  printf("%zu\\n", sizeof(d));']
    lines += [f'  printf("{n} %zu %zu\\n", offsetof(s2m2_segment_desc, {n}), sizeof(d.{n}));' for n in names]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == ctypes.sizeof(hip.SegmentDesc)
    for n, line in zip(names, out[1:]):
        name, off, size = line.split()
        f = getattr(hip.SegmentDesc, n)
        assert (name, int(off), int(size)) == (n, f.offset, f.size)
    assert names == ["cloud", "label", "size", "mask", "disp_out", "stats", "workspace", "max_jump", "min_size"]
    assert hip.SegmentDesc.cloud.size == ctypes.sizeof(hip.CloudDesc)


def test_workspace_size_and_bad_extents(lib):
    """two int32 planes of the image, each in whole 256-byte pieces"""
    for B, H, W in ((1, 1024, 1216), (3, 48, 80), (1, 1, 1), (2, 3, 4100)):
        n = lib.s2m2_segment_workspace_bytes(B, H, W)
        assert n >= 8 * B * H * W and n % 256 == 0 and n - 8 * B * H * W < 512
        assert hip.segment_workspace_bytes(B, H, W) == n
    for B, H, W in ((0, 4, 4), (1, -1, 4), (1, 4, 0), (1, 1 << 15, 1 << 15), (65536, 4, 4)):
        assert lib.s2m2_segment_workspace_bytes(B, H, W) == 0
    assert lib.s2m2_segment_workspace_bytes(1, (1 << 15) - 1, 1 << 15) > 0          # H * W < 2^30
    with pytest.raises(ValueError, match="bad extents"):
        hip.segment_workspace_bytes(1, 0, 4)


def test_tile_is_positive_and_inside_the_image(lib):
    for H, W in ((1, 1), (1, 500), (500, 1), (37, 53), (1024, 1216), (2048, 2432)):
        tr, tc = lib.s2m2_segment_tile_rows(H, W), lib.s2m2_segment_tile_cols(H, W)
        assert 1 <= tr <= H and 1 <= tc <= W
        assert hip.segment_tile(H, W) == (tr, tc)
    big = hip.segment_tile(4096, 4096)
    assert hip.segment_tile(1024, 1216) == big                   # one tile for every image that holds one
    for H, W in ((0, 5), (5, 0), (-1, 5), (1 << 15, 1 << 15)):
        assert lib.s2m2_segment_tile_rows(H, W) == 0 and lib.s2m2_segment_tile_cols(H, W) == 0
    with pytest.raises(ValueError, match="bad extents"):
        hip.segment_tile(0, 5)


BAD = [
    # the input side of s2m2_cloud
    (dict(cloud_disp=None), b"null pointer"),
    (dict(cloud_occ=None), b"null pointer"),
    (dict(cloud_conf=None), b"null pointer"),
    (dict(cloud_H=33), b"larger than the maps"),
    (dict(cloud_W=65), b"larger than the maps"),
    (dict(cloud_B=0), b"non-positive extents"),
    (dict(cloud_H=0), b"non-positive extents"),
    (dict(cloud_W=-3), b"non-positive extents"),
    (dict(cloud_Hp=0), b"non-positive extents"),
    (dict(cloud_Wp=0), b"non-positive extents"),
    (dict(cloud_fx=0.0), b"fx and fy must be positive"),
    (dict(cloud_fy=-1.0), b"fx and fy must be positive"),
    (dict(cloud_depth_scale=0.0), b"depth_scale must be positive"),
    (dict(cloud_image_dtype=3), b"unsupported image dtype"),
    (dict(cloud_disp=4098), b"4-byte aligned"),
    (dict(cloud_H=1 << 16, cloud_W=1 << 15, cloud_Hp=1 << 16, cloud_Wp=1 << 15), b"extents too large"),
    # K22's own
    (dict(cloud_H=1 << 15, cloud_W=1 << 15, cloud_Hp=1 << 15, cloud_Wp=1 << 15), b"segment: extents too large (H*W < 2^30)"),
    (dict(label=None, size=None, mask=None, disp_out=None, stats=None), b"no output requested"),
    (dict(workspace=None), b"null workspace"),
    (dict(workspace=8194), b"workspace must be 4-byte aligned"),
    (dict(label=8193), b"must be 4-byte aligned"),
    (dict(size=8194), b"must be 4-byte aligned"),
    (dict(disp_out=16387), b"must be 4-byte aligned"),
    (dict(stats=8195), b"must be 4-byte aligned"),
    (dict(disp_out=4096), b"disp_out aliases cloud.disp"),
    (dict(max_jump=-0.5), b"max_jump must be >= 0"),
    (dict(max_jump=NAN), b"max_jump must be >= 0"),
    (dict(min_size=0), b"min_size must be 1..2^30"),
    (dict(min_size=-7), b"min_size must be 1..2^30"),
    (dict(min_size=(1 << 30) + 1), b"min_size must be 1..2^30"),
]


@pytest.mark.parametrize("over,msg", BAD, ids=[f"{'-'.join(o)}-{i}" for i, (o, _) in enumerate(BAD)])
def test_validation_fails_before_any_device_call(lib, over, msg):
    assert lib.s2m2_segment(ctypes.byref(_desc(**over)), None) != 0
    assert msg in lib.s2m2_last_error(), lib.s2m2_last_error()
    assert lib.s2m2_last_error().startswith(b"segment: ")


def test_what_is_allowed(lib):
    """a misaligned mask, max_jump = +inf, min_size = 1 and 2^30, a missing image and the ignored output fields of the embedded descriptor pass
    every check: the first failure is the one put there on purpose, which is tested last"""
    d = _desc(mask=8193, max_jump=INF, min_size=1 << 30, cloud_image=None, cloud_capacity=-1, cloud_records=4104, cloud_count=4096,
              cloud_workspace=None, workspace=None)
    assert lib.s2m2_segment(ctypes.byref(d), None) != 0
    assert b"segment: null workspace" in lib.s2m2_last_error(), lib.s2m2_last_error()


def test_null_descriptor(lib):
    assert lib.s2m2_segment(None, None) != 0 and b"null descriptor" in lib.s2m2_last_error()


def test_refused_while_a_plan_records(lib):
    """as K15, K20 and K21: s2m2_segment is not recorded, and says so instead of being silently absent from the plan"""
    plan = ctypes.c_void_p()
    assert lib.s2m2_plan_begin(ctypes.byref(plan)) == 0
    try:
        assert lib.s2m2_segment(ctypes.byref(_desc()), None) != 0
        assert b"not recorded in launch plans" in lib.s2m2_last_error()
        assert lib.s2m2_plan_launches(plan) == 0
    finally:
        lib.s2m2_plan_abort(plan)
        lib.s2m2_plan_destroy(plan)
    header = open(os.path.join(ROOT, "include", "s2m2_hip.h")).read()
    assert "s2m2_segment is NOT recorded" in header


def test_wrappers_reject_bad_operands(lib):
    import torch
    z = torch.zeros(1, 1, 32, 32)
    kw = dict(H=32, W=32, fx=1.0, cx=0.0, cy=0.0, baseline=1.0)
    with pytest.raises(ValueError, match="device tensors"):
        hip.segment(z, z, z, fy=1.0, workspace=torch.zeros(8 * 32 * 32, dtype=torch.uint8), mask=torch.zeros(1, 1, 32, 32, dtype=torch.uint8), **kw)
    for bad, msg in ((dict(max_jump=-1.0), "max_jump must be >= 0"), (dict(max_jump=NAN), "max_jump must be >= 0"),
                     (dict(min_size=0), "min_size must be an integer"), (dict(min_size=2.5), "min_size must be an integer"),
                     (dict(min_size=(1 << 30) + 1), "min_size must be an integer")):
        with pytest.raises(ValueError, match=msg):
            cloud.segment(z, z, z, **kw, **bad)
    with pytest.raises(ValueError, match="device tensors"):
        cloud.segment(z, z, z, **kw)


# ---- the oracle

def _oracle(disp, keep=None, **kw):
    disp = np.asarray(disp, dtype=F)
    conf = np.ones_like(disp) if keep is None else np.asarray(keep, dtype=F)
    return segment_oracle.segment(disp, np.ones_like(disp), conf, **{**CAM, **kw})


def test_oracle_on_hand_computed_5x7_cases():
    # (1) a jump exactly equal to max_jump joins, one above does not.  Rows of constant disparity 10, 11, 12.5, 12.5, 20; max_jump 1:
    # rows 0 and 1 join (|10 - 11| = 1 exactly), row 2 is 1.5 away from row 1, rows 2 and 3 are equal, row 4 is far
    d = np.repeat(np.array([10, 11, 12.5, 12.5, 20], dtype=F)[:, None], 7, axis=1)
    o = _oracle(d, max_jump=1.0)
    assert o["keep"].all()
    assert o["label"].tolist() == [[0] * 7, [0] * 7, [14] * 7, [14] * 7, [28] * 7]
    assert o["size"].tolist() == [[14] * 7, [14] * 7, [14] * 7, [14] * 7, [7] * 7]
    assert o["stats"].tolist() == [35, 3, 35, 3] and o["mask"].all()
    p = _oracle(d, max_jump=1.0, min_size=8)
    assert p["mask"].tolist() == [[1] * 7] * 4 + [[0] * 7] and p["stats"].tolist() == [35, 3, 28, 2]
    assert np.array_equal(p["label"], o["label"]) and np.array_equal(p["size"], o["size"])        # min_size changes the mask alone
    q = _oracle(d, max_jump=np.nextafter(F(1.0), F(0.0)))                                        # just below 1: rows 0 and 1 part
    assert q["label"][:2].tolist() == [[0] * 7, [7] * 7] and q["stats"][1] == 4
    r = _oracle(d, max_jump=1.5)                                                                # 12.5 - 11 = 1.5 exactly: joins
    assert r["label"][:4].tolist() == [[0] * 7] * 4 and r["stats"].tolist() == [35, 2, 35, 2]
    # (2) diagonal neighbours alone do not join: a checkerboard of kept pixels is all singletons, also with max_jump = inf
    k = (np.add.outer(np.arange(5), np.arange(7)) % 2 == 0)
    c = _oracle(np.full((5, 7), 10, F), keep=k, max_jump=INF)
    own = np.arange(35).reshape(5, 7)
    assert np.array_equal(c["keep"], k) and np.array_equal(c["label"], np.where(k, own, -1))
    assert np.array_equal(c["size"], k.astype(np.int32)) and c["stats"].tolist() == [18, 18, 18, 18]
    assert _oracle(np.full((5, 7), 10, F), keep=k, max_jump=INF, min_size=2)["stats"].tolist() == [18, 18, 0, 0]
    # (3) a U: two arms that meet only in the last row are one component, and its label is the first arm's top
    u = np.zeros((5, 7), bool)
    u[:, 1] = u[:, 5] = u[4, 1:6] = True
    c = _oracle(np.full((5, 7), 10, F), keep=u, max_jump=0.0)
    assert np.array_equal(c["label"], np.where(u, 1, -1)) and np.array_equal(c["size"], np.where(u, 13, 0))
    assert c["stats"].tolist() == [13, 1, 13, 1]
    # (4) not kept: low confidence, d <= 0 and non-finite disparities (z = 0 or beyond the truncation); none of them bridges its neighbours
    d = np.full((5, 7), 10, F)
    d[2, :] = [10, -1, NAN, INF, 0, -INF, 10]
    c = _oracle(d, max_jump=INF)
    assert c["keep"][2].tolist() == [True, False, False, False, False, False, True]
    assert c["stats"].tolist() == [30, 1, 30, 1] and (c["label"][c["keep"]] == 0).all()          # joined round the ends of row 2
    d[2, 0] = d[2, 6] = -1
    assert _oracle(d, max_jump=INF)["stats"].tolist() == [28, 2, 28, 2]


def test_oracle_disp_out_keeps_the_maps_own_values_and_fills_the_border():
    g = np.random.default_rng(3)
    dp = g.random((9, 12), dtype=F) + F(5)
    mask = g.random((5, 7)) < 0.5
    out = segment_oracle.disp_out(dp, mask, 5, 7)
    assert out.shape == dp.shape and (out[:2] == -1).all() and (out[7:] == -1).all() and (out[:, :2] == -1).all() and (out[:, 9:] == -1).all()
    win = out[2:7, 2:9]
    assert np.array_equal(win[mask], dp[2:7, 2:9][mask]) and (win[~mask] == -1).all()


@pytest.mark.parametrize("seed,shape,p", [(0, (40, 60), 0.593), (1, (33, 47), 0.5), (2, (200, 330), 0.593), (3, (1, 90), 0.7), (4, (90, 1), 0.7),
                                          (5, (64, 64), 0.95)])
def test_oracle_against_scipy_label(seed, shape, p):
    ndimage = pytest.importorskip("scipy.ndimage")
    g = np.random.default_rng(seed)
    k = g.random(shape) < p
    o = _oracle(np.full(shape, 10, F), keep=k, max_jump=INF)
    lab, n = ndimage.label(k)                                                                   # 4-connectivity is scipy's default
    own = np.arange(k.size).reshape(shape)
    first = np.asarray(ndimage.minimum(own, lab, np.arange(1, n + 1))).astype(np.int64) if n else np.zeros(0, np.int64)
    count = np.bincount(lab.ravel(), minlength=n + 1)
    assert np.array_equal(o["label"], np.where(k, np.concatenate([[-1], first])[lab], -1))
    assert np.array_equal(o["size"], np.where(k, count[lab], 0))
    assert o["stats"].tolist() == [int(k.sum()), n, int(k.sum()), n]


def test_oracle_serpentine_is_one_component():
    H, W = 129, 200
    k = np.zeros((H, W), bool)
    k[0::2] = True
    k[1::4, W - 1] = True
    k[3::4, 0] = True
    o = _oracle(np.full((H, W), 10, F), keep=k, max_jump=0.0)
    assert o["stats"].tolist() == [int(k.sum())] + [1] + [int(k.sum())] + [1] and (o["label"][k] == 0).all()


def test_every_face_of_the_mesh_lies_in_one_component():
    """the face rule of K20 emits a candidate only if its three edges are joined; two of them are axis-aligned, so the three vertices are
    connected through K22's 4-neighbourhood edges"""
    g = np.random.default_rng(11)
    H, W = 60, 90
    disp = (np.add.outer(np.arange(H), np.arange(W)) * 0.4 + g.random((H, W)) * 1.5 + 5).astype(F)
    conf = (g.random((H, W)) < 0.85).astype(F)
    one = np.ones((H, W), F)
    o = segment_oracle.segment(disp, one, conf, max_jump=1.0, **CAM)
    c = cloud_oracle.cloud(disp, one, conf, np.zeros((3, H, W), np.uint8), **CAM)
    assert np.array_equal(c["keep"], o["keep"])
    faces = mesh_oracle.mesh(c["keep"], c["index"], disp, max_jump=1.0)["faces"]
    assert len(faces) > 500 and o["stats"][1] > 20
    lab = o["label"].ravel()[c["index"][faces]]
    assert (lab >= 0).all() and (lab[:, 0] == lab[:, 1]).all() and (lab[:, 1] == lab[:, 2]).all()


# ---- the runner's argument errors (usage errors, before the engine is loaded: no GPU needed)

def test_runner_argument_errors(lib):
    from s2m2_amd.build import RUNNER
    base = [RUNNER, "absent.s2m2", "l.f32", "r.f32"]
    for extra, msg in ((["--min-size", "5"], "--min-size needs --calib"),
                       (["--calib", CALIB, "--min-size", "0", "--ply", "x.ply"], "--min-size: an integer >= 1"),
                       (["--calib", CALIB, "--min-size", "five", "--ply", "x.ply"], "--min-size: an integer >= 1"),
                       (["--calib", CALIB, "--ply", "x.ply", "--labels", "x.i32"], "--labels and --segment-mask need --min-size"),
                       (["--calib", CALIB, "--ply", "x.ply", "--segment-mask", "x.u8"], "--labels and --segment-mask need --min-size"),
                       (["--calib", CALIB, "--ply", "x.ply", "--max-jump", "2"], "--max-jump needs --mesh or --min-size")):
        p = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and msg in p.stderr, (extra, p.stderr)
    # with --min-size, --max-jump and --calib alone are complete: the next failure is the missing engine
    p = subprocess.run(base + ["--calib", CALIB, "--min-size", "5", "--max-jump", "2", "--labels", "x.i32"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "engine_load: cannot open" in p.stderr, p.stderr
