"""CPU-side checks of K21 (include/s2m2_hip.h: s2m2_register, s2m2_amd/cloud.py: register): the boundary (symbols, descriptor layout, ABI version,
workspace sizes, every validation path -- all of which return before any device call, there is no GPU here), the host functions (Camera,
right_camera) and the numpy oracle the GPU tests compare against, on hand-computed pixels and on the two cases of the issue that need no GPU
(the identity target, the right view of an integer-disparity scene)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cloud_oracle
import register_oracle
from s2m2_amd import cloud, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(ROOT, "tests", "golden", "bicycle2_calib.txt")
F = np.float32


@pytest.fixture(scope="module")
def lib():
    from s2m2_amd.build import build
    build(verbose=False)
    return hip.load()


def _desc(**over):
    """a descriptor that passes validation (the pointers are never dereferenced on the host); keys with a `cloud_` prefix go to the embedded
    s2m2_cloud_desc, R / t take a list"""
    d = hip.RegisterDesc()
    c = d.cloud
    c.disp = c.occ = c.conf = c.image = 4096
    c.B, c.H, c.W, c.Hp, c.Wp, c.image_dtype = 1, 30, 50, 32, 64, 2
    c.fx, c.fy, c.cx, c.cy, c.baseline, c.doffs, c.depth_scale, c.depth_trunc, c.conf_min, c.occ_min = 1000.0, 1000.0, 25.0, 15.0, 100.0, 0.0, 1000.0, 3.0, 0.1, 0.5
    d.Ht, d.Wt, d.splat, d.fx_t, d.fy_t, d.cx_t, d.cy_t = 48, 80, 2, 900.0, 910.0, 40.0, 24.0
    d.R = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    d.t = (ctypes.c_double * 3)(0.05, -0.02, 0.03)
    d.depth_t = d.index_t = d.image_t = d.visible = d.count = d.workspace = 4096
    for k, v in over.items():
        if k.startswith("cloud_"):
            setattr(c, k[6:], v)
        elif k in ("R", "t"):
            setattr(d, k, (ctypes.c_double * len(v))(*v))
        else:
            setattr(d, k, v)
    return d


def test_symbols_version_and_header_constant(lib):
    assert hasattr(lib, "s2m2_register") and hasattr(lib, "s2m2_register_workspace_bytes")
    assert "s2m2_register" in hip.SIGNATURES and "s2m2_register_workspace_bytes" in hip.SIGNATURES
    assert lib.s2m2_version() == 800 and hip.ABI_VERSION == 800
    header = open(os.path.join(ROOT, "include", "s2m2_hip.h")).read()
    assert int(re.search(r"#define S2M2_ABI_VERSION (\d+)", header).group(1)) == 800


def test_register_desc_has_the_layout_of_the_header(tmp_path):
    """every field: offset and size of hip.RegisterDesc against s2m2_register_desc compiled by gcc"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = [f[0] for f in hip.RegisterDesc._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "s2m2_hip.h"', "int main(void) {", "  s2m2_register_desc d;",
             '  printf("%zu\\n", sizeof(d));']
    lines += [f'  printf("{n} %zu %zu\\n", offsetof(s2m2_register_desc, {n}), sizeof(d.{n}));' for n in names]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == ctypes.sizeof(hip.RegisterDesc)
    for n, line in zip(names, out[1:]):
        name, off, size = line.split()
        f = getattr(hip.RegisterDesc, n)
        assert (name, int(off), int(size)) == (n, f.offset, f.size)
    assert hip.RegisterDesc.cloud.size == ctypes.sizeof(hip.CloudDesc)


def test_workspace_size(lib):
    """one 8-byte key per target pixel, in whole 256-byte pieces"""
    for B, Ht, Wt in ((1, 1024, 1216), (3, 48, 80), (1, 1, 1), (2, 3, 4100)):
        n = lib.s2m2_register_workspace_bytes(B, Ht, Wt)
        assert n >= 8 * B * Ht * Wt and n % 256 == 0 and n - 8 * B * Ht * Wt < 256
        assert hip.register_workspace_bytes(B, Ht, Wt) == n
    assert lib.s2m2_register_workspace_bytes(0, 4, 4) == 0 and lib.s2m2_register_workspace_bytes(1, -1, 4) == 0
    assert lib.s2m2_register_workspace_bytes(1, 4, 0) == 0 and lib.s2m2_register_workspace_bytes(1, 1 << 16, 1 << 15) == 0
    with pytest.raises(ValueError, match="bad extents"):
        hip.register_workspace_bytes(1, 0, 4)


NAN, INF = float("nan"), float("inf")
EYE = [1, 0, 0, 0, 1, 0, 0, 0, 1]
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
    # the target
    (dict(Ht=0), b"non-positive target extents"),
    (dict(Wt=-1), b"non-positive target extents"),
    (dict(Ht=1 << 16, Wt=1 << 15), b"target extents too large"),
    (dict(fx_t=0.0), b"fx_t and fy_t must be positive"),
    (dict(fy_t=-2.0), b"fx_t and fy_t must be positive"),
    (dict(fx_t=1e-60), b"fx_t and fy_t must be positive"),           # positive, but 0 in fp32
    (dict(splat=0), b"splat must be 1..4"),
    (dict(splat=5), b"splat must be 1..4"),
    (dict(fx_t=INF), b"must be finite"),
    (dict(cy_t=NAN), b"must be finite"),
    (dict(cx_t=1e300), b"must be finite"),                           # finite, but inf in fp32
    (dict(R=[1, 0, 0, 0, NAN, 0, 0, 0, 1]), b"must be finite"),
    (dict(R=[1, 0, 0, 0, 1, 0, 0, 0, -INF]), b"must be finite"),
    (dict(t=[0, INF, 0]), b"must be finite"),
    (dict(t=[0, 0, NAN]), b"must be finite"),
    # outputs and workspace
    (dict(depth_t=None, index_t=None, image_t=None, visible=None, count=None), b"no output requested"),
    (dict(cloud_image=None), b"null pointer (cloud.image) while image_t is requested"),
    (dict(workspace=None), b"null workspace"),
    (dict(workspace=4100), b"workspace must be 8-byte aligned"),
    (dict(depth_t=4098), b"must be 4-byte aligned"),
    (dict(index_t=4097), b"must be 4-byte aligned"),
    (dict(count=4099), b"must be 4-byte aligned"),
]


@pytest.mark.parametrize("over,msg", BAD, ids=[f"{'-'.join(o)}-{i}" for i, (o, _) in enumerate(BAD)])
def test_validation_fails_before_any_device_call(lib, over, msg):
    assert lib.s2m2_register(ctypes.byref(_desc(**over)), None) != 0
    assert msg in lib.s2m2_last_error(), lib.s2m2_last_error()


def test_the_output_fields_of_the_embedded_descriptor_are_ignored(lib):
    """a negative capacity, a misaligned records pointer and a count without workspace are errors of s2m2_cloud; here they are not looked at:
    with an otherwise valid descriptor the first failure is the one put there on purpose, behind every check of the embedded descriptor"""
    d = _desc(cloud_capacity=-1, cloud_records=4104, cloud_count=4096, cloud_workspace=None, workspace=None)
    assert lib.s2m2_register(ctypes.byref(d), None) != 0
    assert b"register: null workspace" in lib.s2m2_last_error(), lib.s2m2_last_error()


def test_null_descriptor(lib):
    assert lib.s2m2_register(None, None) != 0 and b"null descriptor" in lib.s2m2_last_error()


def test_refused_while_a_plan_records(lib):
    """as K15: s2m2_register is not recorded, and says so instead of being silently absent from the plan"""
    plan = ctypes.c_void_p()
    assert lib.s2m2_plan_begin(ctypes.byref(plan)) == 0
    try:
        assert lib.s2m2_register(ctypes.byref(_desc()), None) != 0
        assert b"not recorded in launch plans" in lib.s2m2_last_error()
        assert lib.s2m2_plan_launches(plan) == 0
    finally:
        lib.s2m2_plan_abort(plan)
        lib.s2m2_plan_destroy(plan)
    header = open(os.path.join(ROOT, "include", "s2m2_hip.h")).read()
    assert "s2m2_register is NOT recorded" in header


def test_binding_rejects_host_tensors(lib):
    import torch
    z = torch.zeros(1, 1, 32, 32)
    img = torch.zeros(1, 3, 32, 32, dtype=torch.uint8)
    cam = cloud.Camera(32, 32, 1.0, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="device tensors"):
        cloud.register(z, z, z, img, fx=1.0, cx=0.0, cy=0.0, baseline=1.0, to=cam)
    with pytest.raises(ValueError, match="device tensors"):
        hip.register(z, z, z, img, fx=1.0, fy=1.0, cx=0.0, cy=0.0, baseline=1.0, Ht=32, Wt=32, fx_t=1.0, fy_t=1.0, cx_t=0.0, cy_t=0.0, R=EYE,
                     t=[0, 0, 0], workspace=torch.zeros(8 * 32 * 32, dtype=torch.uint8), depth_t=torch.zeros(1, 1, 32, 32))


def test_camera_and_right_camera_on_the_fixture():
    c = cloud.read_calib_file(CALIB)
    cam = cloud.right_camera(c, 2852, 1952)
    assert (cam.width, cam.height) == (2852, 1952)
    assert (cam.fx, cam.fy, cam.cx, cam.cy) == (3896.34, 3896.34, 1228.699, 976.456)
    assert np.array_equal(cam.R, np.eye(3)) and cam.t.tolist() == [-173.557 / 1000.0, 0.0, 0.0]
    assert cloud.right_camera(c, 10, 20, depth_scale=1.0).t.tolist() == [-173.557, 0.0, 0.0]
    d = cloud.Camera(8, 6, 2.0, 3.0, 4.0, 5.0)
    assert np.array_equal(d.R, np.eye(3)) and d.t.tolist() == [0.0, 0.0, 0.0] and d.R.dtype == np.float64
    e = cloud.Camera(8, 6, 2.0, 3.0, 4.0, 5.0, R=list(range(9)), t=(1, 2, 3))
    assert e.R.shape == (3, 3) and e.R[1, 2] == 5.0 and e.t.tolist() == [1.0, 2.0, 3.0]


def test_oracle_on_hand_computed_pixels():
    """2x3 source; fx = fy = 1000, baseline 100, doffs 0, depth_scale 1000 (z = 100 / disp m), cx = cy = 0; identity pose; target 2x2 with
    fx_t = fy_t = 300, cx_t = cy_t = 0, splat 1: up = 300 * (u * z / 1000) / z = 0.3 u up to rounding, so floor(up + 0.5) is 0 for u = 0, 1
    (0.5, 0.8) and 1 for u = 2 (1.1), far from any integer; likewise rows 0, 1 -> target row 0.
      row 0: disp 50 (z = 2) | 50 (z = 2) | 50 (z = 2)          row 1: disp 25 (z = 4) | 50 (z = 2), low confidence | 100 (z = 1)
    Target (0,0) receives source pixels 0 and 1 at equal Z = 2 (the lower index, 0, wins) and pixel 3 at Z = 4 (farther: loses).
    Target (0,1) receives pixel 2 (Z = 2) and pixel 5 (Z = 1, nearer: wins).  Row 1 of the target is empty.  Pixel 4 is not kept (its sentinel depth of 1e6 m
    lies beyond the truncation at 10 m)."""
    disp = np.array([[50, 50, 50], [25, 50, 100]], dtype=F)
    conf = np.array([[1, 1, 1], [1, 0.05, 1]], dtype=F)
    occ = np.ones((2, 3), dtype=F)
    img = (np.arange(18, dtype=np.uint8).reshape(3, 2, 3) + 1) * 10
    kw = dict(fx=1000.0, fy=1000.0, cx=0.0, cy=0.0, baseline=100.0, doffs=0.0, depth_trunc=10.0)
    tgt = dict(Ht=2, Wt=2, fx_t=300.0, fy_t=300.0, cx_t=0.0, cy_t=0.0)
    o = register_oracle.register(disp, occ, conf, img, splat=1, **tgt, **kw)
    assert o["index_t"].tolist() == [[0, 5], [-1, -1]]
    assert o["depth_t"].tolist() == [[2.0, 1.0], [0.0, 0.0]]
    assert o["visible"].tolist() == [[1, 0, 0], [0, 0, 1]]
    assert o["count"] == 2
    assert o["image_t"][:, 0, 0].tolist() == [10, 70, 130] and o["image_t"][:, 0, 1].tolist() == [60, 120, 180]
    assert not o["image_t"][:, 1].any()
    # the two colliding pixels really had equal Z bits, and swapping their order in memory cannot matter: the key carries the index
    assert o["keep"].tolist() == [[True, True, True], [True, False, True]]
    # a translation of +1 m along z: Z = z + 1 and up = 0.3 u z / (z + 1) <= 0.4: everything lands on target (0,0), the nearest is pixel 5
    p = register_oracle.register(disp, occ, conf, img, splat=1, t=[0, 0, 1.0], **tgt, **kw)
    assert p["depth_t"].tolist() == [[2.0, 0.0], [0.0, 0.0]] and p["index_t"].tolist() == [[5, -1], [-1, -1]] and p["count"] == 1
    # splat 2 around up = (0, 0.3, 0.6), vp = (0, 0.3): c = 0, origin (0, 0) for every pixel, footprint = the whole 2x2 target; the
    # nearest surface (pixel 5, Z = 1) takes all four
    q = register_oracle.register(disp, occ, conf, img, splat=2, **tgt, **kw)
    assert q["index_t"].tolist() == [[5, 5], [5, 5]] and q["count"] == 4 and q["visible"].sum() == 1
    # behind the camera: a rotation of 180 degrees about y turns every Z negative
    r = register_oracle.register(disp, occ, conf, img, splat=2, R=[-1, 0, 0, 0, 1, 0, 0, 0, -1], **tgt, **kw)
    assert r["count"] == 0 and (r["index_t"] == -1).all() and not r["depth_t"].any() and not r["visible"].any()


def _calib():
    c = cloud.read_calib_file(CALIB)
    return dict(fx=float(c["cam0"][0, 0]), fy=float(c["cam0"][1, 1]), cx=float(c["cam0"][0, 2]), cy=float(c["cam0"][1, 2]),
                baseline=float(c["baseline"]), doffs=float(c["doffs"]))


@pytest.mark.parametrize("trunc", [3.0, None])
def test_oracle_identity_target_returns_the_depth_map(trunc):
    """R = I, t = 0, cam0's intrinsics, the source's size, splat 1: every kept pixel lands on itself -- (fx * x) / z + cx rounds back to u with
    an error far below the half pixel of the footprint -- and Z = ((x*0 + y*0) + z) + 0 = z bit for bit, also for the 1e6 m sentinel points"""
    H, W = 1000, 1190
    k = _calib()
    g = np.random.default_rng(5)
    disp = (g.random((H, W), dtype=F) * F(320.0) - F(20.0)).astype(F)
    conf, occ = g.random((H, W), dtype=F), g.random((H, W), dtype=F)
    o = register_oracle.register(disp, occ, conf, None, Ht=H, Wt=W, fx_t=k["fx"], fy_t=k["fy"], cx_t=k["cx"], cy_t=k["cy"], splat=1,
                                 depth_trunc=trunc, **k)
    ref = cloud_oracle.cloud(disp, occ, conf, np.zeros((3, H, W), np.uint8), depth_trunc=trunc, **k)
    own = np.arange(H * W, dtype=np.int32).reshape(H, W)
    assert np.array_equal(o["index_t"], np.where(ref["keep"], own, -1))
    assert np.array_equal(o["depth_t"].view(np.int32), ref["depth"].view(np.int32))
    assert np.array_equal(o["visible"].astype(bool), ref["keep"]) and o["count"] == int(ref["keep"].sum())
    if trunc is None:
        assert o["count"] > 0.3 * H * W and (o["depth_t"] == F(1e6)).any()


def test_oracle_right_view_is_the_painters_algorithm():
    H, W = 24, 96
    k = dict(fx=1000.0, fy=1000.0, cx=50.0, cy=10.0, baseline=100.0, doffs=0.0)
    disp, index, visible = register_oracle.right_view_scene(H, W)
    one = np.ones((H, W), dtype=F)
    o = register_oracle.register(disp, one, one, None, Ht=H, Wt=W, fx_t=k["fx"], fy_t=k["fy"], cx_t=k["cx"], cy_t=k["cy"],
                                 t=[-k["baseline"] / 1000.0, 0, 0], splat=1, depth_trunc=None, **k)
    assert np.array_equal(o["index_t"], index)
    assert np.array_equal(o["visible"], visible)
    # invisible: exactly the background pixels that leave the image (u < 8) or that the rectangle hides
    hidden = np.zeros((H, W), dtype=bool)
    hidden[:, :8] = True
    r0, r1, c0, c1 = H // 4, 3 * H // 4, W // 2, 3 * W // 4
    hidden[r0:r1, c0 - 40 + 8:c1 - 40 + 8] = True
    hidden[r0:r1, c0:c1] = False                                     # the rectangle itself is seen whole
    assert np.array_equal(o["visible"] == 0, hidden)
    # the holes sit at the disocclusion (right of the shifted rectangle) and at the right border
    holes = o["index_t"] == -1
    assert holes[:, W - 8:].all() and holes[r0:r1, c0 - 8:c1 - 8].all() and holes.sum() == 8 * H + (r1 - r0) * (c1 - c0)
