"""CPU-side checks of the 3D output stage (K15: include/s2m2_hip.h s2m2_cloud, s2m2_amd/cloud.py): the boundary (symbols, descriptor layout, ABI
version, every validation path -- all of which return before any device call, there is no GPU here), the host functions (calibration file,
PLY writer) and the numpy oracle the GPU tests compare against, on hand-computed pixels."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cloud_oracle
from s2m2_amd import cloud, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(ROOT, "tests", "golden", "bicycle2_calib.txt")


@pytest.fixture(scope="module")
def lib():
    from s2m2_amd.build import build
    build(verbose=False)
    return hip.load()


def _desc(**over):
    """a descriptor that passes validation (the pointers are never dereferenced on the host)"""
    d = hip.CloudDesc()
    d.disp = d.occ = d.conf = d.image = d.depth = d.mask = d.records = d.count = d.workspace = 4096
    d.B, d.H, d.W, d.Hp, d.Wp, d.image_dtype, d.capacity = 1, 30, 50, 32, 64, 2, 1500
    d.fx, d.fy, d.cx, d.cy, d.baseline, d.doffs, d.depth_scale, d.depth_trunc, d.conf_min, d.occ_min = 1000.0, 1000.0, 25.0, 15.0, 100.0, 0.0, 1000.0, 3.0, 0.1, 0.5
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_symbols_version_and_header_constant(lib):
    assert hasattr(lib, "s2m2_cloud") and hasattr(lib, "s2m2_cloud_workspace_bytes")
    assert "s2m2_cloud" in hip.SIGNATURES and "s2m2_cloud_workspace_bytes" in hip.SIGNATURES
    assert lib.s2m2_version() == 800 and hip.ABI_VERSION == 800
    header = open(os.path.join(ROOT, "include", "s2m2_hip.h")).read()
    assert int(re.search(r"#define S2M2_ABI_VERSION (\d+)", header).group(1)) == 800


def test_cloud_desc_has_the_layout_of_the_header(tmp_path):
    """every field: offset and size of hip.CloudDesc against s2m2_cloud_desc compiled by gcc"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = [f[0] for f in hip.CloudDesc._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "s2m2_hip.h"', "int main(void) {", "  s2m2_cloud_desc d;",
             '  printf("%zu\\n", sizeof(d));']
    lines += [f'  printf("{n} %zu %zu\\n", offsetof(s2m2_cloud_desc, {n}), sizeof(d.{n}));' for n in names]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == ctypes.sizeof(hip.CloudDesc)
    for n, line in zip(names, out[1:]):
        name, off, size = line.split()
        f = getattr(hip.CloudDesc, n)
        assert (name, int(off), int(size)) == (n, f.offset, f.size)


def test_workspace_size(lib):
    assert lib.s2m2_cloud_workspace_bytes(1, 1024, 1216) >= 4 * -(-1024 // 3)              # 3 rows of 1216 pixels per tile
    assert lib.s2m2_cloud_workspace_bytes(3, 2000, 2400) >= 4 * 3 * 2000
    assert lib.s2m2_cloud_workspace_bytes(1, 1, 1) >= 4
    assert lib.s2m2_cloud_workspace_bytes(0, 4, 4) == 0 and lib.s2m2_cloud_workspace_bytes(1, -1, 4) == 0 and lib.s2m2_cloud_workspace_bytes(1, 4, 0) == 0


BAD = [
    (dict(disp=None), b"null pointer"),
    (dict(occ=None), b"null pointer"),
    (dict(conf=None), b"null pointer"),
    (dict(image=None), b"null pointer (image)"),
    (dict(records=None), b"null pointer (records)"),
    (dict(depth=None, mask=None, count=None), b"no output requested"),
    (dict(H=33), b"larger than the maps"),
    (dict(W=65), b"larger than the maps"),
    (dict(B=0), b"non-positive extents"),
    (dict(H=0), b"non-positive extents"),
    (dict(W=-3), b"non-positive extents"),
    (dict(Hp=0), b"non-positive extents"),
    (dict(Wp=0), b"non-positive extents"),
    (dict(fx=0.0), b"fx and fy must be positive"),
    (dict(fy=-1.0), b"fx and fy must be positive"),
    (dict(depth_scale=0.0), b"depth_scale must be positive"),
    (dict(capacity=-1), b"negative capacity"),
    (dict(image_dtype=3), b"unsupported image dtype"),
    (dict(image_dtype=-1), b"unsupported image dtype"),
    (dict(workspace=None), b"null workspace while a cloud is requested"),
    (dict(records=4104), b"16-byte aligned"),
]


@pytest.mark.parametrize("over,msg", BAD, ids=[f"{'-'.join(o)}-{i}" for i, (o, _) in enumerate(BAD)])
def test_validation_fails_before_any_device_call(lib, over, msg):
    assert lib.s2m2_cloud(ctypes.byref(_desc(**over)), None) != 0
    assert msg in lib.s2m2_last_error(), lib.s2m2_last_error()


def test_null_descriptor(lib):
    assert lib.s2m2_cloud(None, None) != 0 and b"null descriptor" in lib.s2m2_last_error()


def test_refused_while_a_plan_records(lib):
    """the header's choice for launch plans: s2m2_cloud is not recorded, and says so instead of being silently absent from the plan"""
    plan = ctypes.c_void_p()
    assert lib.s2m2_plan_begin(ctypes.byref(plan)) == 0
    try:
        assert lib.s2m2_cloud(ctypes.byref(_desc()), None) != 0
        assert b"not recorded in launch plans" in lib.s2m2_last_error()
        assert lib.s2m2_plan_launches(plan) == 0
    finally:
        lib.s2m2_plan_abort(plan)
        lib.s2m2_plan_destroy(plan)
    header = open(os.path.join(ROOT, "include", "s2m2_hip.h")).read()
    assert "s2m2_cloud is NOT recorded" in header


def test_binding_rejects_host_tensors():
    import torch
    z = torch.zeros(1, 1, 32, 32)
    with pytest.raises(ValueError, match="device tensors"):
        cloud.reproject(z, z, z, torch.zeros(1, 3, 32, 32, dtype=torch.uint8), fx=1.0, cx=0.0, cy=0.0, baseline=1.0)


def test_read_calib_file_on_the_fixture():
    c = cloud.read_calib_file(CALIB)
    assert c["cam0"].shape == (3, 3) and c["cam1"].shape == (3, 3)
    assert c["cam0"][0, 0] == 3896.34 and c["cam0"][0, 2] == 1064.836 and c["cam0"][1, 2] == 976.456 and c["cam0"][1, 1] == 3896.34
    assert c["cam1"][0, 2] == 1228.699 and c["cam0"][2, 2] == 1.0
    assert c["doffs"] == 163.863 and c["baseline"] == 173.557
    assert (c["width"], c["height"], c["ndisp"]) == (2852.0, 1952.0, 250.0)


def test_ply_writer_round_trip(tmp_path):
    rec = np.zeros(5, dtype=cloud.RECORD_DTYPE)
    rec["x"], rec["y"], rec["z"] = [0.5, -1.25, 3.0, 1e-3, -7.0], [1.0, 2.0, -3.0, 4.0, 0.0], [2.0, 2.5, 0.75, 1.0, 2.9990001]
    rec["red"], rec["green"], rec["blue"], rec["alpha"] = [0, 1, 127, 254, 255], [9, 8, 7, 6, 5], [255, 0, 255, 0, 13], 255
    path = str(tmp_path / "five.ply")
    assert cloud.write_ply_records(path, rec) == 5
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert head.decode().split("\n")[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 5"]
    assert [ln.split()[1:] for ln in head.decode().split("\n") if ln.startswith("property")] == \
        [["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"], ["uchar", "green"], ["uchar", "blue"], ["uchar", "alpha"]]
    assert body == rec.tobytes() and len(body) == 80
    back = cloud.read_ply_records(path)
    assert back.tobytes() == rec.tobytes()
    # the same buffer as the device holds it: (n, 4) int32
    assert cloud.write_ply_records(str(tmp_path / "i32.ply"), rec.view(np.int32).reshape(5, 4)) == 5
    assert open(tmp_path / "i32.ply", "rb").read() == raw
    with pytest.raises(ValueError):
        cloud.write_ply_records(str(tmp_path / "bad.ply"), b"123")


def test_oracle_on_hand_computed_pixels():
    """fx = fy = 1000, baseline 100, doffs 0, depth_scale 1000: depth = 1e5 / disp mm, z = 100 / disp m; cx = 2, cy = 1; trunc 3 m.
    One row of six pixels at v = 1 (so y = 0 everywhere) -- except that the principal-point pixel sits at u = 2:
      u=0 kept: disp 50 -> z = 2, x = (0-2)*2/1000 = -0.004        u=1 low confidence (0.05)       u=2 principal point: disp 100 -> z = 1, x = y = 0
      u=3 occluded (occ 0.4)         u=4 disp = 0 -> sentinel 1e9 / 1000 = 1e6 m, beyond 3 m         u=5 disp 20 -> z = 5 m, beyond 3 m
    and a row v = 0 above it with one kept pixel (u=4, disp 40 -> z = 2.5, x = (4-2)*2.5/1000 = 0.005, y = (0-1)*2.5/1000 = -0.0025)."""
    disp = np.array([[-3, -3, -3, -3, 40, -3], [50, 50, 100, 50, 0, 20]], dtype=np.float32)
    conf = np.array([[1, 1, 1, 1, 1, 1], [1, 0.05, 1, 1, 1, 1]], dtype=np.float32)
    occ = np.array([[1, 1, 1, 1, 1, 1], [1, 1, 1, 0.4, 1, 1]], dtype=np.float32)
    img = np.arange(36, dtype=np.uint8).reshape(3, 2, 6) * 7
    kw = dict(fx=1000.0, fy=1000.0, cx=2.0, cy=1.0, baseline=100.0, doffs=0.0, depth_trunc=3.0)
    o = cloud_oracle.cloud(disp, occ, conf, img, **kw)
    assert o["keep"].tolist() == [[False, False, False, False, True, False], [True, False, True, False, False, False]]
    assert o["index"].tolist() == [4, 6, 8]                                     # raster order
    assert o["z"].tolist() == [2.5, 2.0, 1.0]
    assert o["depth"].tolist() == [[0, 0, 0, 0, 2.5, 0], [2.0, 0, 1.0, 0, 0, 0]]
    np.testing.assert_allclose(o["x64"], [0.005, -0.004, 0.0], rtol=0, atol=1e-18)
    np.testing.assert_allclose(o["y64"], [-0.0025, 0.0, 0.0], rtol=0, atol=1e-18)
    assert o["x32"].tolist() == [np.float32(0.005), np.float32(-0.004), 0.0] and o["y32"].dtype == np.float32
    assert o["rgb"].tolist() == [[28, 112, 196], [42, 126, 210], [56, 140, 224]]
    # unfiltered: the low-confidence and the occluded pixel come back (disp 50 -> z = 2), nothing else changes
    u = cloud_oracle.cloud(disp, occ, conf, img, filtered=False, **kw)
    assert u["index"].tolist() == [4, 6, 7, 8, 9] and u["z"].tolist() == [2.5, 2.0, 2.0, 1.0, 2.0]
    # no truncation (1e9, the reference's None): the 1e9 mm sentinel is 1e6 m and passes, as it does in the reference -- every pixel is a point
    n = cloud_oracle.cloud(disp, occ, conf, img, **dict(kw, depth_trunc=None))
    assert n["keep"].all() and n["z"][0] == 1e6 and n["z"][11] == 5.0
    # doffs enters the denominator; float images round half to even and clamp
    d = cloud_oracle.cloud(disp, occ, conf, img, **dict(kw, doffs=50.0))
    assert d["z"].tolist()[:3] == [np.float32(1e5) / np.float32(90) / np.float32(1000), 1.0, np.float32(1e5) / np.float32(150) / np.float32(1000)]
    f = np.array([0.5, 1.5, 2.5, -4.0, 254.5, 300.0], dtype=np.float32)
    assert cloud_oracle.colour_bytes(f).tolist() == [0, 2, 2, 0, 254, 255]
    # the crop window of image_crop
    m = np.arange(32 * 64).reshape(1, 32, 64)
    assert cloud_oracle.crop(m, 30, 50)[0, 0, 0] == 1 * 64 + 7 and cloud_oracle.crop(m, 30, 50).shape == (1, 30, 50)
    assert cloud_oracle.crop(m, 1, 1)[0, 0, 0] == 15 * 64 + 31
