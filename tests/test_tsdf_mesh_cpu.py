"""CPU-side checks of K25 (include/s2m2_hip.h: s2m2_tsdf_mesh; s2m2_amd/mc_table.py; s2m2_amd/cloud.py: TsdfVolume.extract_mesh): the generated
case table (coverage, agreement of the two cells that share a face, the committed header), the numpy oracle the GPU tests compare against
(against a scalar triple loop, against tsdf_oracle's points, on volumes whose surface is a closed oriented manifold), and the boundary: symbols,
descriptor layout, workspace size, every validation path -- all of which return before any device call, there is no GPU here --, the wrappers'
own errors and the runner's option rules."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tsdf_mesh_oracle as M
import tsdf_oracle as O
import tsdf_scenes as S
from s2m2_amd import cloud, hip, mc_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(ROOT, "tests", "golden", "bicycle2_calib.txt")
F = np.float32
NAN = float("nan")
PLACE = dict(origin=(0.0, 0.0, 0.0), voxel_size=1.0)                  # positions in voxels


@pytest.fixture(scope="module")
def lib():
    from s2m2_amd.build import build
    build(verbose=False)
    return hip.load()


def volume(t, weight=None):
    """(Nz, Ny, Nx) tsdf values (and weights, default 1) -> a volume with colours that differ from voxel to voxel"""
    t = np.asarray(t, F)
    vol = O.empty(t.shape[::-1])
    vol[..., 0] = t.view(np.int32)
    vol[..., 1] = 1 if weight is None else weight
    lin = np.arange(t.size, dtype=np.int64).reshape(t.shape)
    vol[..., 2] = ((lin * 37) % 65281 | ((lin * 101) % 65281) << 16).astype(np.int32)
    vol[..., 3] = ((lin * 53) % 65281).astype(np.int32)
    return vol


# ---- the case table

def test_table_statistics_and_coverage():
    table = mc_table.build_table()
    assert len(table) == 256 and table[0] == [] and table[255] == []
    assert mc_table.max_triangles(table) == 5 and sum(len(t) for t in table) == 820
    assert sorted({len(loop) for case in range(256) for loop in mc_table.case_loops(case)}) == [3, 4, 5, 6, 7]
    for case, tris in enumerate(table):
        changing = {e for e in range(12) if mc_table.changing(case, e)}
        used = set()
        for tri in tris:
            assert len(set(tri)) == 3 and set(tri) <= changing, (case, tri)
            used |= set(tri)
        assert used == changing, case
    assert mc_table.EDGES == [(0, 0), (0, 2), (0, 4), (0, 6), (1, 0), (1, 1), (1, 4), (1, 5), (2, 0), (2, 1), (2, 2), (2, 3)]


def _directed_in_face(tris, f, s):
    """the directed triangle edges (pairs of edge numbers) whose two ends both lie in cube face (f, s)"""
    fe = set(mc_table.face_edges(f, s))
    return sorted((a, b) for tri in tris for a, b in zip(tri, tri[1:] + tri[:1]) if a in fe and b in fe)


def test_table_shared_faces():
    """3 axes x 256 cases x 16 neighbours that agree on the shared face's signs: the triangle edges lying in the face are exactly its segments,
    and the neighbour has each of them reversed"""
    table = mc_table.build_table()
    number = {ab: e for e, ab in enumerate(mc_table.EDGES)}
    pairs = 0
    for f in range(3):
        low = [c for c in range(8) if not c >> f & 1]
        across = {number[(a, b)]: number[(a, b ^ 1 << f)] for a, b in mc_table.EDGES if a != f and b >> f & 1}   # this cell's edge -> the neighbour's
        back = {v: k for k, v in across.items()}
        for case in range(256):
            mine = _directed_in_face(table[case], f, 1)
            segments = sorted(tuple(sorted(sg)) for sg in mc_table.face_segments(case, f, 1))
            assert sorted(tuple(sorted(d)) for d in mine) == segments, (f, case)
            shared = sum((case >> (c | 1 << f) & 1) << c for c in low)
            for rest in range(16):
                other = shared | sum((rest >> n & 1) << (c | 1 << f) for n, c in enumerate(low))
                theirs = sorted((back[b], back[a]) for a, b in _directed_in_face(table[other], f, 0))             # reversed, in this cell's numbers
                assert theirs == mine, (f, case, other)
                pairs += 1
    assert pairs == 3 * 256 * 16


def test_the_committed_header_is_the_generators_output():
    assert open(mc_table.HEADER, "rb").read() == mc_table.header_text().encode("ascii")
    text = mc_table.header_text()
    assert "GENERATED" in text and "kMcMaxTriangles = 5;" in text and "kMcRowBytes = 16;" in text


# ---- the oracle

def _scalar_mesh(vol, min_weight):
    """K25's definition voxel by voxel and cell by cell, with Python loops -> (list of (lin, axis) per vertex, list of faces)"""
    Nz, Ny, Nx, _ = vol.shape
    u = O.unpack(vol)
    t, w = u["tsdf"], u["weight"]
    stride = (1, Nx, Nx * Ny)
    rank, points = {}, []
    for k in range(Nz):
        for j in range(Ny):
            for i in range(Nx):
                lin = (k * Ny + j) * Nx + i
                for a, inside in enumerate((i + 1 < Nx, j + 1 < Ny, k + 1 < Nz)):
                    if inside and w[lin] >= min_weight and w[lin + stride[a]] >= min_weight and (t[lin] < 0) != (t[lin + stride[a]] < 0):
                        rank[(lin, a)] = len(points)
                        points.append((lin, a))
    faces = []
    for k in range(Nz - 1):
        for j in range(Ny - 1):
            for i in range(Nx - 1):
                lin = (k * Ny + j) * Nx + i
                corner = [lin + (c & 1) + (c >> 1 & 1) * Nx + (c >> 2) * Nx * Ny for c in range(8)]
                if any(w[v] < min_weight for v in corner):
                    continue
                case = sum(int(t[v] < 0) << c for c, v in enumerate(corner))
                for tri in M.TABLE[case]:
                    faces.append([rank[(corner[mc_table.EDGES[e][1]], mc_table.EDGES[e][0])] for e in tri])
    return points, faces


@pytest.mark.parametrize("min_weight", [1, 2])
def test_oracle_against_a_scalar_triple_loop(min_weight):
    g = np.random.default_rng(5)
    t = g.uniform(-1, 1, (5, 6, 7)).astype(F)
    t[g.random(t.shape) < 0.05] = 0.0
    t[0, 0, 0] = -0.0
    vol = volume(t, np.where(g.random(t.shape) < 0.08, g.integers(0, 2, t.shape), 3))          # a few unobserved, some seen once
    m = M.mesh(vol, **PLACE, min_weight=min_weight)
    points, faces = _scalar_mesh(vol, min_weight)
    assert m["count"] == len(points) > 50 and list(zip(m["lin"].tolist(), m["axis"].tolist())) == points
    assert m["face_count"] == len(faces) > 20 and m["faces"].tolist() == faces and m["faces"].dtype == np.int32
    assert not m["valid"].all() and m["valid"].any()


def test_the_vertices_are_extracts_points():
    g = np.random.default_rng(6)
    t = g.uniform(-1, 1, (6, 5, 9)).astype(F)
    vol = volume(t, np.where(g.random(t.shape) < 0.08, g.integers(0, 2, t.shape), 3))
    for min_weight in (1, 2):
        m = M.mesh(vol, origin=(-0.3, 0.2, 1.5), voxel_size=0.05, min_weight=min_weight)
        e = O.extract(vol, origin=(-0.3, 0.2, 1.5), voxel_size=0.05, min_weight=min_weight)
        assert m["count"] == e["count"] > 0 and m["records"].tobytes() == e["records"].tobytes()
        assert m["gradients"].view(np.int32).tobytes() == e["gradients"].view(np.int32).tobytes()
        referenced = np.unique(m["faces"])
        assert referenced.min() >= 0 and referenced.max() < e["count"] and len(referenced) < e["count"]      # some points lie on no face


def _sphere(n, centre, r):
    k, j, i = np.indices((n, n, n)).astype(np.float64)
    return np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2 + (k - centre[2]) ** 2) - r


SPHERE_R = 4.2


def _closed_volumes():
    sphere = _sphere(14, (6.3, 6.6, 6.4), SPHERE_R)
    blobs = np.minimum(_sphere(16, (4.3, 4.4, 4.6), 2.65), _sphere(16, (11.2, 10.7, 11.4), 2.75))
    noise = np.random.default_rng(1).uniform(-1, 1, (12, 12, 12))
    inner = np.zeros(noise.shape, bool)
    inner[1:-1, 1:-1, 1:-1] = True
    noise[~inner] = np.abs(noise[~inner]) + 0.01
    return dict(sphere=sphere, blobs=blobs, noise=noise)


def _manifold_numbers(m):
    """asserts that every directed edge occurs exactly once and its reverse exactly once -> (signed volume, V - E + F)"""
    f = m["faces"].astype(np.int64)
    n = m["count"]
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    assert (directed[:, 0] != directed[:, 1]).all()
    key, back = directed[:, 0] * n + directed[:, 1], directed[:, 1] * n + directed[:, 0]
    assert len(np.unique(key)) == len(key), "a directed edge occurs twice"
    assert np.array_equal(np.sort(key), np.sort(back)), "a directed edge has no reverse"
    p = m["records"][:, :3].view(F).astype(np.float64)
    vol6 = np.einsum("ij,ij->i", p[f[:, 0]], np.cross(p[f[:, 1]], p[f[:, 2]])).sum()
    return vol6 / 6.0, len(np.unique(f)) - len(key) // 2 + len(f)


@pytest.mark.parametrize("name", ["sphere", "blobs", "noise"])
def test_closed_oriented_manifolds(name):
    t = _closed_volumes()[name]
    outer = np.ones(t.shape, bool)
    outer[1:-1, 1:-1, 1:-1] = False
    assert (t[outer] > 0).all() and (t < 0).any() and (t != 0).all()
    m = M.mesh(volume(t), **PLACE)
    assert m["valid"].all() and m["face_count"] > 100
    signed_volume, euler = _manifold_numbers(m)
    assert signed_volume > 0
    if name == "sphere":
        assert euler == 2
        assert 4 / 3 * np.pi * (SPHERE_R - 1) ** 3 < signed_volume < 4 / 3 * np.pi * (SPHERE_R + 1) ** 3
        g = m["gradients"].astype(np.float64)                           # the faces look where the gradients point
        p = m["records"][:, :3].view(F).astype(np.float64)
        f = m["faces"]
        normal = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
        assert (np.einsum("ij,ij->i", normal, g[f[:, 0]]) > 0).mean() > 0.95
    if name == "blobs":
        assert euler == 4
    if name == "noise":
        assert len(np.unique(m["case"])) > 200


def test_one_unobserved_voxel_removes_the_faces_of_its_eight_cells():
    t = _closed_volumes()["sphere"]
    vol = volume(t)
    hole = (6, 6, 10)                                                   # (k, j, i): next to the surface
    before = M.mesh(vol, **PLACE)
    vol[hole][1] = 0
    after = M.mesh(vol, **PLACE)
    Nz, Ny, Nx = t.shape
    around = {((hole[0] - dz) * Ny + hole[1] - dy) * Nx + hole[2] - dx for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
    keep = ~np.isin(before["face_cell"], list(around))
    assert 0 < keep.sum() < len(keep) and after["face_count"] == keep.sum() and after["count"] < before["count"]
    assert np.array_equal(after["face_cell"], before["face_cell"][keep])
    assert before["records"][before["faces"][keep]].tobytes() == after["records"][after["faces"]].tobytes()       # the same vertices, renumbered


def test_a_fused_scene_has_a_mesh():
    grid = S.GRID_LONG
    poses = np.array([S.IDENTITY, S.rot_xy(0.1, -0.15, (0.05, -0.03, 0.1))], F)
    vol, _ = O.integrate(O.empty(grid["dims"]), *S.frames(["steps", "tilt"]), poses, origin=grid["origin"], voxel_size=grid["voxel_size"],
                         trunc=grid["trunc"], max_weight=64, **S.CAM)
    m = M.mesh(vol, origin=grid["origin"], voxel_size=grid["voxel_size"])
    assert m["face_count"] > 0 and m["faces"].min() >= 0 and m["faces"].max() < m["count"]
    assert m["face_count"] <= 4 * m["count"]                            # the bound the runner sizes its face buffer by
    assert not m["valid"].all()


def test_grids_with_an_extent_of_one_have_no_cells():
    t = np.random.default_rng(2).uniform(-1, 1, (40, 13, 1)).astype(F)
    m = M.mesh(volume(t), **PLACE)
    assert m["face_count"] == 0 and m["faces"].shape == (0, 3) and m["count"] > 100


# ---- the boundary

def _mdesc(**over):
    """a mesh descriptor that passes validation (the pointers are never dereferenced on the host)"""
    d = hip.TsdfMeshDesc()
    x = d.extract
    x.volume, x.records, x.gradients, x.count, x.workspace = 1 << 20, 1 << 21, 1 << 22, 8192, 16384
    x.Nx, x.Ny, x.Nz, x.min_weight, x.capacity = 19, 13, 11, 1, 100
    x.origin = (ctypes.c_double * 3)(-1.0, -1.0, 0.5)
    x.voxel_size = 0.05
    d.faces, d.face_count, d.face_capacity = 1 << 23, 4096, 50
    for k, v in over.items():
        if k.startswith("origin"):
            x.origin[int(k[6:])] = v
        else:
            setattr(d if k in ("faces", "face_count", "face_capacity") else x, k, v)
    return d


def test_symbols_version_and_header(lib):
    for name in ("s2m2_tsdf_mesh", "s2m2_tsdf_mesh_workspace_bytes"):
        assert hasattr(lib, name) and name in hip.SIGNATURES
    assert lib.s2m2_version() == 800 and hip.ABI_VERSION == 800
    header = open(os.path.join(ROOT, "include", "s2m2_hip.h")).read()
    assert int(re.search(r"#define S2M2_ABI_VERSION (\d+)", header).group(1)) == 800
    assert "s2m2_tsdf_mesh is NOT recorded" in header


def test_desc_has_the_layout_of_the_header(tmp_path):
    """every field: offset and size of the ctypes mirror against the struct compiled by gcc"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = [f[0] for f in hip.TsdfMeshDesc._fields_]
    assert names == ["extract", "faces", "face_count", "face_capacity"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "s2m2_hip.h"', "int main(void) {", "  s2m2_tsdf_mesh_desc d;",
             '  printf("%zu\\n", sizeof(d));']
    lines += [f'  printf("{n} %zu %zu\\n", offsetof(s2m2_tsdf_mesh_desc, {n}), sizeof(d.{n}));' for n in names]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == ctypes.sizeof(hip.TsdfMeshDesc)
    for n, line in zip(names, out[1:]):
        field, off, size = line.split()
        f = getattr(hip.TsdfMeshDesc, n)
        assert (field, int(off), int(size)) == (n, f.offset, f.size)


LIMIT = (2 ** 31 - 1) // 5


def test_workspace_and_the_size_limit(lib):
    def r256(n):
        return -(-n // 256) * 256
    for dims in ((19, 13, 11), (1, 1, 1), (512, 512, 512), (37, 21, 23), (LIMIT, 1, 1)):
        n = dims[0] * dims[1] * dims[2]
        tiles = -(-n // lib.s2m2_tsdf_tile_voxels(*dims))
        assert lib.s2m2_tsdf_mesh_workspace_bytes(*dims) == r256(8 * tiles) + r256(4 * n) == hip.tsdf_mesh_workspace_bytes(*dims)
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (1024, 1024, 512), (1 << 30, 1, 1), (LIMIT + 1, 1, 1), (1024, 1024, 410)):
        assert lib.s2m2_tsdf_mesh_workspace_bytes(*dims) == 0
    assert lib.s2m2_tsdf_workspace_bytes(1024, 1024, 410) > 0           # K24 takes what K25's int32 face count refuses
    with pytest.raises(ValueError, match="bad extents"):
        hip.tsdf_mesh_workspace_bytes(1024, 1024, 410)


MBAD = [
    # what s2m2_tsdf_extract checks
    (dict(volume=None), b"null pointer (volume)"),
    (dict(volume=(1 << 20) + 4), b"volume must be 16-byte aligned"),
    (dict(Nx=0), b"non-positive dims"),
    (dict(Nx=1024, Ny=1024, Nz=512), b"dims too large"),
    (dict(voxel_size=0.0), b"voxel_size must be finite and > 0"),
    (dict(voxel_size=NAN), b"voxel_size must be finite and > 0"),
    (dict(origin1=NAN), b"origin must be finite"),
    (dict(min_weight=0), b"min_weight must be >= 1"),
    (dict(capacity=-1), b"negative capacity"),
    (dict(records=None, gradients=None), b"null pointers (records and gradients) with capacity 100"),
    (dict(records=(1 << 21) + 8), b"records must be 16-byte aligned"),
    (dict(gradients=(1 << 22) + 2), b"must be 4-byte aligned"),
    (dict(count=8193), b"must be 4-byte aligned"),
    # K25's own
    (dict(face_count=None), b"null pointer (face_count)"),
    (dict(face_count=4098), b"faces and face_count must be 4-byte aligned"),
    (dict(faces=(1 << 23) + 1), b"faces and face_count must be 4-byte aligned"),
    (dict(face_capacity=-1), b"negative face_capacity"),
    (dict(faces=None), b"null pointer (faces) with face_capacity 50"),
    (dict(Nx=1024, Ny=1024, Nz=410), b"dims too large for an int32 face count"),
    (dict(Nx=LIMIT + 1, Ny=1, Nz=1), b"dims too large for an int32 face count"),
    (dict(workspace=None), b"null workspace"),
    (dict(workspace=16386), b"workspace must be 4-byte aligned"),
]


@pytest.mark.parametrize("over,msg", MBAD, ids=[f"{'-'.join(o)}-{i}" for i, (o, _) in enumerate(MBAD)])
def test_validation_fails_before_any_device_call(lib, over, msg):
    assert lib.s2m2_tsdf_mesh(ctypes.byref(_mdesc(**over)), None) != 0
    assert msg in lib.s2m2_last_error(), lib.s2m2_last_error()
    assert lib.s2m2_last_error().startswith(b"tsdf_mesh: ")


def test_what_is_allowed(lib):
    """a faces-only call, a count-only call, each vertex output alone, the largest volume: the first failure is the one put there on purpose"""
    for over in (dict(records=None, gradients=None, count=None, capacity=0), dict(faces=None, face_capacity=0), dict(gradients=None),
                 dict(records=None), dict(count=None), dict(Nx=LIMIT, Ny=1, Nz=1), dict(records=None, gradients=None, count=None, capacity=0,
                                                                                      faces=None, face_capacity=0)):
        assert lib.s2m2_tsdf_mesh(ctypes.byref(_mdesc(workspace=None, **over)), None) != 0
        assert b"tsdf_mesh: null workspace" in lib.s2m2_last_error(), lib.s2m2_last_error()


def test_null_descriptor(lib):
    assert lib.s2m2_tsdf_mesh(None, None) != 0 and b"tsdf_mesh: null descriptor" in lib.s2m2_last_error()


def test_refused_while_a_plan_records(lib):
    plan = ctypes.c_void_p()
    assert lib.s2m2_plan_begin(ctypes.byref(plan)) == 0
    try:
        assert lib.s2m2_tsdf_mesh(ctypes.byref(_mdesc()), None) != 0
        assert b"not recorded in launch plans" in lib.s2m2_last_error()
        assert lib.s2m2_plan_launches(plan) == 0
    finally:
        lib.s2m2_plan_abort(plan)
        lib.s2m2_plan_destroy(plan)


def test_wrappers_reject_bad_operands(lib):
    import torch
    tv = cloud.TsdfVolume((4, 5, 6), 0.1, (0.0, 0.0, 1.0), device="cpu")
    with pytest.raises(ValueError, match="negative capacity"):
        tv.extract_mesh(capacity=-1)
    with pytest.raises(ValueError, match="negative capacity"):
        tv.extract_mesh(face_capacity=-1)
    vol = torch.zeros(6, 5, 4, 4, dtype=torch.int32)
    ws = torch.zeros(1024, dtype=torch.uint8)
    with pytest.raises(ValueError, match="device tensors"):
        hip.tsdf_mesh(vol, origin=(0, 0, 0), voxel_size=0.1, workspace=ws, face_count=torch.zeros(1, dtype=torch.int32))
    assert issubclass(cloud.TsdfMesh, cloud.TsdfSurface)
    m = cloud.TsdfMesh(torch.zeros(1, 7, 4, dtype=torch.int32), torch.tensor([3], dtype=torch.int32), None, torch.zeros(9, 3, dtype=torch.int32),
                       torch.tensor([12], dtype=torch.int32))
    assert m.face_capacity() == 9 and m.face_size() == 9 and tuple(m.faces().shape) == (9, 3) and m.size() == 3
    m.count[0] = 8
    with pytest.raises(ValueError, match="unstored vertices"):
        m.faces()


def test_ply_mesh_with_normals_round_trip(tmp_path):
    g = np.random.default_rng(3)
    rec = np.zeros(5, cloud.NORMAL_RECORD_DTYPE)
    for name in ("x", "y", "z", "nx", "ny", "nz"):
        rec[name] = g.normal(size=5).astype(F)
    rec["red"], rec["alpha"] = [1, 2, 3, 4, 5], 255
    faces = np.array([[0, 1, 2], [2, 1, 4]], np.int32)
    assert cloud.write_ply_mesh(str(tmp_path / "n.ply"), rec, faces, normals=True) == (5, 2)
    got, f = cloud.read_ply_mesh(str(tmp_path / "n.ply"))
    assert got.dtype == cloud.NORMAL_RECORD_DTYPE and got.tobytes() == rec.tobytes() and np.array_equal(f, faces)
    assert b"property float nx" in open(tmp_path / "n.ply", "rb").read()
    plain = np.zeros(5, cloud.RECORD_DTYPE)
    assert cloud.write_ply_mesh(str(tmp_path / "p.ply"), plain, faces) == (5, 2)
    got, f = cloud.read_ply_mesh(str(tmp_path / "p.ply"))
    assert got.dtype == cloud.RECORD_DTYPE and np.array_equal(f, faces)
    with pytest.raises(ValueError, match="28-byte records"):
        cloud.write_ply_mesh(str(tmp_path / "x.ply"), plain, faces, normals=True)


# ---- the runner's option rules (usage errors, before the engine is loaded: no GPU needed)

def test_runner_tsdf_mesh_rules(lib, tmp_path):
    from s2m2_amd.build import RUNNER
    good = tmp_path / "list.txt"
    good.write_text("l0.f32 r0.f32 i0.u8 1 0 0 0 0 1 0 0 0 0 1 0\n")
    full = ["--tsdf-frames", str(good), "--tsdf-dims", "19,13,11", "--tsdf-voxel", "0.1", "--tsdf-origin", "-0.9,-0.6,1.5", "--calib", CALIB,
            "--tsdf-ply", "t.ply", "--tsdf-mesh", "m.ply"]

    def run(args):
        p = subprocess.run([RUNNER] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert p.returncode != 0 and p.stderr.startswith("s2m2_run_engine: ") and p.stderr.count("\n") == 1, p.stderr
        return p.stderr

    def drop(flag):
        i = full.index(flag)
        return full[:i] + full[i + 2:]

    assert "engine_load: cannot open" in run(["absent.s2m2"] + full)            # complete: the next failure is the missing engine
    assert "need --tsdf-frames" in run(["absent.s2m2", "--tsdf-mesh", "m.ply"])
    assert "need --tsdf-frames" in run(["absent.s2m2"] + drop("--tsdf-frames"))
    assert "--tsdf-frames needs --tsdf-dims, --tsdf-voxel, --tsdf-origin, --calib and --tsdf-ply" in run(["absent.s2m2"] + drop("--tsdf-ply"))
    assert "comes without the options of a single pair" in run(["absent.s2m2"] + full + ["--mesh", "x.ply"])
    big = list(full)
    big[big.index("--tsdf-dims") + 1] = "1024,1024,410"
    assert "--tsdf-mesh: NX*NY*NZ <= 429496729" in run(["absent.s2m2"] + big)
    assert "engine_load: cannot open" in run(["absent.s2m2"] + [a for a in big if a not in ("--tsdf-mesh", "m.ply")])
    assert "--tsdf-mesh" in subprocess.run([RUNNER], capture_output=True, text=True, timeout=60).stderr          # the usage line names it
