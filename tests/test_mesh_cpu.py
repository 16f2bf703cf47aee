"""CPU-side checks of the surface mesh stage (K20: include/s2m2_hip.h s2m2_mesh, s2m2_amd/cloud.py): the boundary (symbols, descriptor layout,
ABI version, every validation path -- all of which return before any device call, there is no GPU here), the host functions (PLY mesh writer and
reader) and the numpy oracle the GPU tests compare against, on hand-written grids with the expected faces written out."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mesh_oracle
from s2m2_amd import cloud, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from s2m2_amd.build import build
    build(verbose=False)
    return hip.load()


def _desc(**over):
    """a descriptor that passes validation (the pointers are never dereferenced on the host); cloud_<field> sets a field of the nested descriptor"""
    d = hip.MeshDesc()
    c = d.cloud
    c.disp = c.occ = c.conf = c.image = c.depth = c.mask = c.records = c.count = c.workspace = 4096
    c.B, c.H, c.W, c.Hp, c.Wp, c.image_dtype, c.capacity = 1, 30, 50, 32, 64, 2, 1500
    c.fx, c.fy, c.cx, c.cy, c.baseline, c.doffs, c.depth_scale, c.depth_trunc, c.conf_min, c.occ_min = 1000.0, 1000.0, 25.0, 15.0, 100.0, 0.0, 1000.0, 3.0, 0.1, 0.5
    d.faces = d.face_count = d.index = 8192
    d.face_capacity, d.max_jump = 2 * 29 * 49, 1.0
    for k, v in over.items():
        if k.startswith("cloud_"):
            setattr(c, k[6:], v)
        else:
            setattr(d, k, v)
    return d


def test_symbols_version_and_header(lib):
    for name in ("s2m2_mesh", "s2m2_mesh_workspace_bytes", "s2m2_mesh_tile_rows"):
        assert hasattr(lib, name) and name in hip.SIGNATURES
    assert lib.s2m2_version() == 800 and hip.ABI_VERSION == 800
    header = open(os.path.join(ROOT, "include", "s2m2_hip.h")).read()
    assert int(re.search(r"#define S2M2_ABI_VERSION (\d+)", header).group(1)) == 800
    assert "typedef struct s2m2_mesh_desc" in header and "s2m2_mesh is NOT recorded" in header


def test_mesh_desc_has_the_layout_of_the_header(tmp_path):
    """every field, the nested cloud descriptor's included: offset and size of hip.MeshDesc against s2m2_mesh_desc compiled by gcc"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    top = [f[0] for f in hip.MeshDesc._fields_]
    nested = [f[0] for f in hip.CloudDesc._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "s2m2_hip.h"', "int main(void) {", "  s2m2_mesh_desc d;",
             '  printf("%zu\\n", sizeof(d));']
    lines += [f'  printf("{n} %zu %zu\\n", offsetof(s2m2_mesh_desc, {n}), sizeof(d.{n}));' for n in top]
    lines += [f'  printf("cloud.{n} %zu %zu\\n", offsetof(s2m2_mesh_desc, cloud.{n}), sizeof(d.cloud.{n}));' for n in nested]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == ctypes.sizeof(hip.MeshDesc)
    assert top == ["cloud", "faces", "face_count", "index", "face_capacity", "max_jump"]
    for n, line in zip(top, out[1:]):
        name, off, size = line.split()
        f = getattr(hip.MeshDesc, n)
        assert (name, int(off), int(size)) == (n, f.offset, f.size)
    base = hip.MeshDesc.cloud.offset
    for n, line in zip(nested, out[1 + len(top):]):
        name, off, size = line.split()
        f = getattr(hip.CloudDesc, n)
        assert (name, int(off), int(size)) == ("cloud." + n, base + f.offset, f.size)


def test_workspace_and_tile_rows(lib):
    # the workspace holds two counts per tile and, without `index`, the dense rank map
    for B, H, W in ((1, 1024, 1216), (3, 2000, 2400), (1, 1, 1), (2, 37, 61)):
        rows = lib.s2m2_mesh_tile_rows(H, W)
        assert rows == max(1, 2048 // W)                                     # whole rows, about 2048 pixels
        assert lib.s2m2_mesh_workspace_bytes(B, H, W) >= 4 * B * H * W + 8 * B * -(-H // rows)
    assert lib.s2m2_mesh_tile_rows(1024, 1216) == 1 and lib.s2m2_mesh_tile_rows(3, 4100) == 1 and lib.s2m2_mesh_tile_rows(140, 61) == 33
    assert lib.s2m2_mesh_workspace_bytes(0, 4, 4) == 0 and lib.s2m2_mesh_workspace_bytes(1, -1, 4) == 0 and lib.s2m2_mesh_workspace_bytes(1, 4, 0) == 0
    assert lib.s2m2_mesh_workspace_bytes(70000, 4, 4) == 0
    assert lib.s2m2_mesh_workspace_bytes(1, 1 << 15, 1 << 15) == 0            # H*W = 2^30: the face count would not fit an int32
    assert lib.s2m2_mesh_tile_rows(0, 4) == 0 and lib.s2m2_mesh_tile_rows(4, -1) == 0 and lib.s2m2_mesh_tile_rows(1 << 15, 1 << 15) == 0
    with pytest.raises(ValueError, match="bad extents"):
        hip.mesh_workspace_bytes(1, 0, 5)
    with pytest.raises(ValueError, match="bad extents"):
        hip.mesh_tile_rows(0, 5)
    assert hip.mesh_tile_rows(1000, 1190) == 1 and hip.mesh_tile_rows(375, 500) == 4


BAD = [
    # what s2m2_cloud checks, through the nested descriptor
    (dict(cloud_disp=None), b"mesh: null pointer (disp / occ / conf)"),
    (dict(cloud_occ=None), b"mesh: null pointer"),
    (dict(cloud_conf=None), b"mesh: null pointer"),
    (dict(cloud_image=None), b"mesh: null pointer (image)"),
    (dict(cloud_records=None), b"mesh: null pointer (records)"),
    (dict(cloud_H=33), b"larger than the maps"),
    (dict(cloud_W=65), b"larger than the maps"),
    (dict(cloud_B=0), b"mesh: non-positive extents"),
    (dict(cloud_H=0), b"non-positive extents"),
    (dict(cloud_W=-3), b"non-positive extents"),
    (dict(cloud_Hp=0), b"non-positive extents"),
    (dict(cloud_Wp=0), b"non-positive extents"),
    (dict(cloud_B=65536), b"extents too large"),
    (dict(cloud_fx=0.0), b"fx and fy must be positive"),
    (dict(cloud_fy=-1.0), b"fx and fy must be positive"),
    (dict(cloud_depth_scale=0.0), b"depth_scale must be positive"),
    (dict(cloud_capacity=-1), b"negative capacity"),
    (dict(cloud_image_dtype=3), b"unsupported image dtype"),
    (dict(cloud_workspace=None), b"mesh: null workspace while a cloud is requested (s2m2_mesh_workspace_bytes)"),
    (dict(cloud_workspace=4098), b"workspace must be 4-byte aligned"),
    (dict(cloud_records=4104), b"16-byte aligned"),
    (dict(cloud_disp=4097), b"fp32 tensors must be 4-byte aligned"),
    # the mesh's own
    (dict(cloud_count=None), b"mesh: face_count comes with count"),
    (dict(cloud_H=1 << 15, cloud_W=1 << 15, cloud_Hp=1 << 15, cloud_Wp=1 << 15), b"mesh: extents too large (H*W < 2^30)"),
    (dict(face_capacity=-1), b"mesh: negative face_capacity -1"),
    (dict(faces=None), b"mesh: null pointer (faces) with face_capacity"),
    (dict(faces=8194), b"must be 4-byte aligned"),
    (dict(index=8193), b"must be 4-byte aligned"),
    (dict(face_count=8195), b"must be 4-byte aligned"),
    (dict(max_jump=-0.5), b"mesh: max_jump must be >= 0"),
    (dict(max_jump=float("nan")), b"mesh: max_jump must be >= 0"),
    (dict(max_jump=float("-inf")), b"mesh: max_jump must be >= 0"),
]


@pytest.mark.parametrize("over,msg", BAD, ids=[f"{'-'.join(o)}-{i}" for i, (o, _) in enumerate(BAD)])
def test_validation_fails_before_any_device_call(lib, over, msg):
    assert lib.s2m2_mesh(ctypes.byref(_desc(**over)), None) != 0
    assert msg in lib.s2m2_last_error(), lib.s2m2_last_error()


def test_null_descriptor(lib):
    assert lib.s2m2_mesh(None, None) != 0 and b"mesh: null descriptor" in lib.s2m2_last_error()


def test_without_face_count_the_call_is_s2m2_cloud(lib):
    """face_count NULL: no mesh is requested, the nested descriptor goes to s2m2_cloud -- seen here through its validation messages"""
    assert lib.s2m2_mesh(ctypes.byref(_desc(face_count=None, cloud_image=None)), None) != 0
    assert b"cloud: null pointer (image)" in lib.s2m2_last_error()


def test_refused_while_a_plan_records(lib):
    plan = ctypes.c_void_p()
    assert lib.s2m2_plan_begin(ctypes.byref(plan)) == 0
    try:
        assert lib.s2m2_mesh(ctypes.byref(_desc()), None) != 0
        assert b"mesh: s2m2_mesh is not recorded in launch plans" in lib.s2m2_last_error()
        assert lib.s2m2_mesh(ctypes.byref(_desc(face_count=None)), None) != 0          # the forwarded form is refused as well
        assert b"not recorded in launch plans" in lib.s2m2_last_error()
        assert lib.s2m2_plan_launches(plan) == 0
    finally:
        lib.s2m2_plan_abort(plan)
        lib.s2m2_plan_destroy(plan)


def test_binding_rejects_host_tensors():
    import torch
    from s2m2_amd import utils
    z = torch.zeros(1, 1, 32, 32)
    img = torch.zeros(1, 3, 32, 32, dtype=torch.uint8)
    with pytest.raises(ValueError, match="device tensors"):
        cloud.mesh(z, z, z, img, fx=1.0, cx=0.0, cy=0.0, baseline=1.0)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
    with pytest.raises(ValueError, match="device tensors"):
        hip.mesh(z, z, z, img, fx=1.0, fy=1.0, cx=0.0, cy=0.0, baseline=1.0, records=i32(1, 4, 4), count=i32(1), faces=i32(1, 4, 3),
                 face_count=i32(1), workspace=torch.zeros(1 << 16, dtype=torch.uint8))
    assert callable(utils.get_mesh)


def test_ply_mesh_round_trip(tmp_path):
    rec = np.zeros(5, dtype=cloud.RECORD_DTYPE)
    rec["x"], rec["y"], rec["z"] = [0.5, -1.25, 3.0, 1e-3, -7.0], [1.0, 2.0, -3.0, 4.0, 0.0], [2.0, 2.5, 0.75, 1.0, 2.9990001]
    rec["red"], rec["green"], rec["blue"], rec["alpha"] = [0, 1, 127, 254, 255], [9, 8, 7, 6, 5], [255, 0, 255, 0, 13], 255
    faces = np.array([[0, 2, 3], [0, 3, 1], [1, 3, 4]], dtype=np.int32)
    path = str(tmp_path / "five.ply")
    assert cloud.write_ply_mesh(path, rec, faces) == (5, 3)
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().split("\n")
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 5"]
    assert lines[-3:] == ["element face 3", "property list uchar int vertex_indices", ""]
    assert len(body) == 5 * 16 + 3 * 13 and body[:80] == rec.tobytes()
    assert body[80:] == b"".join(b"\x03" + f.astype("<i4").tobytes() for f in faces)
    r, f = cloud.read_ply_mesh(path)
    assert r.tobytes() == rec.tobytes() and f.dtype == np.int32 and f.tolist() == faces.tolist()
    # int64 faces (the oracle's) and the device layout of the records
    assert cloud.write_ply_mesh(str(tmp_path / "i64.ply"), rec.view(np.int32).reshape(5, 4), faces.astype(np.int64)) == (5, 3)
    assert open(tmp_path / "i64.ply", "rb").read() == raw
    # zero faces, zero vertices
    assert cloud.write_ply_mesh(str(tmp_path / "nofaces.ply"), rec, np.zeros((0, 3), np.int32)) == (5, 0)
    r, f = cloud.read_ply_mesh(str(tmp_path / "nofaces.ply"))
    assert r.tobytes() == rec.tobytes() and f.shape == (0, 3)
    assert cloud.write_ply_mesh(str(tmp_path / "empty.ply"), b"", np.zeros((0, 3), np.int32)) == (0, 0)
    r, f = cloud.read_ply_mesh(str(tmp_path / "empty.ply"))
    assert len(r) == 0 and f.shape == (0, 3)
    with pytest.raises(ValueError):
        cloud.write_ply_mesh(str(tmp_path / "bad.ply"), b"123", faces)
    with pytest.raises(ValueError, match="outside"):
        cloud.write_ply_mesh(str(tmp_path / "bad.ply"), rec, np.array([[0, 1, 5]]))
    with pytest.raises(ValueError):
        cloud.write_ply_mesh(str(tmp_path / "bad.ply"), rec, np.array([[0, 1]]))
    cloud.write_ply_records(str(tmp_path / "points.ply"), rec)
    with pytest.raises(ValueError):
        cloud.read_ply_mesh(str(tmp_path / "points.ply"))


def _faces(keep, disp, max_jump=1.0):
    keep = np.array(keep, dtype=bool)
    o = mesh_oracle.mesh(keep, np.flatnonzero(keep.ravel()), np.array(disp, dtype=np.float32), max_jump)
    return o["faces"].tolist(), o


ALL22 = [[1, 1], [1, 1]]
NAN = float("nan")


def test_oracle_on_2x2_grids():
    """ranks with all four kept: a=0 b=1 c=2 e=3"""
    # a tie (0 <= 0) takes the diagonal a-e: (a,c,e) then (a,e,b)
    f, o = _faces(ALL22, [[7, 7], [7, 7]])
    assert f == [[0, 2, 3], [0, 3, 1]]
    assert o["hist"]["kept4_tie"] == 1 and o["hist"]["kept4_diag_ae"] == 1 and o["hist"]["quads_2_faces"] == 1 and o["hist"]["emit_tie"] == 1
    assert o["rank"].tolist() == [[0, 1], [2, 3]]
    # |da-de| = 1 > |db-dc| = 0: the diagonal b-c: (a,c,b) then (b,c,e)
    f, o = _faces(ALL22, [[0, .5], [.5, 1]])
    assert f == [[0, 2, 1], [1, 2, 3]] and o["hist"]["kept4_diag_bc"] == 1 and o["hist"]["emit4_acb"] == 1 and o["hist"]["emit4_bce"] == 1
    # |da-de| = 0.25 < |db-dc| = 0.5: a-e without a tie
    f, o = _faces(ALL22, [[0, .5], [0, .25]])
    assert f == [[0, 2, 3], [0, 3, 1]] and o["hist"]["kept4_tie"] == 0
    # three kept, every missing corner (ranks follow the raster order of the three)
    assert _faces([[1, 1], [1, 0]], [[3, 3], [3, 3]])[0] == [[0, 2, 1]]              # e missing: (a,c,b)
    assert _faces([[0, 1], [1, 1]], [[3, 3], [3, 3]])[0] == [[0, 1, 2]]              # a missing: (b,c,e)
    assert _faces([[1, 0], [1, 1]], [[3, 3], [3, 3]])[0] == [[0, 1, 2]]              # b missing: (a,c,e)
    assert _faces([[1, 1], [0, 1]], [[3, 3], [3, 3]])[0] == [[0, 2, 1]]              # c missing: (a,e,b)
    f, o = _faces([[1, 1], [0, 1]], [[3, 3], [3, 3]])
    assert o["hist"]["kept3_miss_c"] == 1 and o["hist"]["emit3_aeb"] == 1 and o["hist"]["quads_1_face"] == 1 and o["rank"].tolist() == [[0, 1], [-1, 2]]
    # three kept but one edge of the triangle is not joined: nothing
    assert _faces([[1, 1], [1, 0]], [[3, 3], [9, 3]])[0] == []
    # the disparity of a pixel that is not kept plays no part
    assert _faces([[1, 1], [1, 0]], [[3, 3], [3, NAN]])[0] == [[0, 2, 1]]
    # fewer than three
    for keep in ([[1, 0], [0, 1]], [[1, 1], [0, 0]], [[0, 0], [0, 1]], [[0, 0], [0, 0]]):
        f, o = _faces(keep, [[3, 3], [3, 3]])
        assert f == [] and o["hist"]["kept_fewer"] == 1 and o["hist"]["quads_0_faces"] == 1
    # an edge of exactly max_jump is joined (<=); just below it is not.  d_a-d_e = d_b-d_c = 1: a tie, a-e
    f, o = _faces(ALL22, [[0, 1], [0, 1]], 1.0)
    assert f == [[0, 2, 3], [0, 3, 1]] and o["hist"]["edge_at_max_jump"] == 4      # ab, ce (the last row), ae, bc
    assert _faces(ALL22, [[0, 1], [0, 1]], 0.999)[0] == []
    # four kept, one candidate only.  a-e: (a,c,e) loses its edge a-c, (a,e,b) stays
    f, o = _faces(ALL22, [[0, 0], [5, 0]])
    assert f == [[0, 3, 1]] and o["hist"]["emit4_aeb"] == 1 and o["hist"]["emit4_ace"] == 0 and o["hist"]["quads_1_face"] == 1
    # b-c: (b,c,e) loses c-e, (a,c,b) stays; and the other way round
    assert _faces(ALL22, [[0, 0], [0, 5]])[0] == [[0, 2, 1]]
    assert _faces(ALL22, [[5, 0], [0, 0]])[0] == [[1, 2, 3]]
    # a NaN among four kept corners (keep forced): the comparison of the diagonals is false -> b-c, and every edge at the NaN is not joined
    assert _faces(ALL22, [[NAN, 0], [0, 0]])[0] == [[1, 2, 3]]
    assert _faces(ALL22, [[0, NAN], [0, 0]])[0] == []
    # max_jump 0: equal disparities only; +inf: every kept neighbour (but inf - inf is NaN)
    assert _faces(ALL22, [[2, 2], [2, 2]], 0.0)[0] == [[0, 2, 3], [0, 3, 1]]
    assert _faces(ALL22, [[2, 2], [2, 2.25]], 0.0)[0] == [[0, 2, 1]]
    assert _faces(ALL22, [[0, 100], [-50, 1e6]], float("inf"))[0] == [[0, 2, 1], [1, 2, 3]]
    # a = b = -inf: both diagonals are inf long (a tie: a-e); a-c and a-e are inf <= inf, a-b is NaN: (a,c,e) stays, (a,e,b) goes
    assert _faces(ALL22, [[float("-inf"), float("-inf")], [0, 1]], float("inf"))[0] == [[0, 2, 3]]
    assert _faces(ALL22, [[float("-inf"), float("-inf")], [float("-inf"), float("-inf")]], float("inf"))[0] == []


def test_oracle_on_2x3_and_3x3_grids():
    # 2x3, ranks 0 1 2 / 3 4 5.  quad 0: a tie -> (0,3,4), (0,4,1).  quad 1 (a=1 b=2 c=4 e=5): |1-e| = 9 > 0 -> b-c, (a,c,b) = (1,4,2) stays,
    # (b,c,e) loses c-e
    f, o = _faces([[1, 1, 1], [1, 1, 1]], [[0, 0, 0], [0, 0, 9]])
    assert f == [[0, 3, 4], [0, 4, 1], [1, 4, 2]]
    assert o["hist"]["quads_2_faces"] == 1 and o["hist"]["quads_1_face"] == 1 and o["hist"]["kept4_diag_bc"] == 1
    # 3x3 without its centre, ranks 0 1 2 / 3 - 4 / 5 6 7: every three-corner case once, in raster order of the quads
    keep = [[1, 1, 1], [1, 0, 1], [1, 1, 1]]
    f, o = _faces(keep, np.zeros((3, 3)))
    assert f == [[0, 3, 1], [1, 4, 2], [3, 5, 6], [4, 6, 7]]
    assert [o["hist"][k] for k in ("kept3_miss_e", "kept3_miss_c", "kept3_miss_b", "kept3_miss_a")] == [1, 1, 1, 1]
    assert o["rank"].tolist() == [[0, 1, 2], [3, -1, 4], [5, 6, 7]]
    # 3x3 all kept on a ramp of 0.5 px per column and row: |da-de| = 1 > |db-dc| = 0 everywhere -> b-c; eight faces
    ramp = [[0, .5, 1], [.5, 1, 1.5], [1, 1.5, 2]]
    f, o = _faces(np.ones((3, 3)), ramp)
    assert f == [[0, 3, 1], [1, 3, 4], [1, 4, 2], [2, 4, 5], [3, 6, 4], [4, 6, 7], [4, 7, 5], [5, 7, 8]]
    # the same ramp with max_jump 0.25: no edge is joined
    assert _faces(np.ones((3, 3)), ramp, 0.25)[0] == []
    # a vertex no face references is still a vertex: the isolated corner keeps its rank
    f, o = _faces([[1, 0, 1], [0, 1, 1], [1, 1, 1]], np.zeros((3, 3)))
    assert o["rank"].tolist() == [[0, -1, 1], [-1, 2, 3], [4, 5, 6]] and f == [[1, 2, 3], [2, 4, 5], [2, 5, 6], [2, 6, 3]]
    # rows or columns of one pixel: vertices, no quads
    f, o = _faces([[1, 1, 1]], [[0, 0, 0]])
    assert f == [] and o["rank"].tolist() == [[0, 1, 2]]
