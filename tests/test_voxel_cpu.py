"""CPU-side checks of K23 (include/s2m2_hip.h: s2m2_voxel, s2m2_amd/cloud.py: voxelize): the boundary (symbols, descriptor layout, workspace
size, the exported hash, every validation path -- all of which return before any device call, there is no GPU here), the wrappers' own errors,
the runner's option rules, and the numpy oracle the GPU tests compare against, checked against a brute-force Python dictionary that uses
floor division, the remainder and exact fractions instead of shifts, masks and the rounding formula."""
import ctypes
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import cloud_oracle
import voxel_oracle
from s2m2_amd import cloud, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(ROOT, "tests", "golden", "bicycle2_calib.txt")
F = np.float32
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from s2m2_amd.build import build
    build(verbose=False)
    return hip.load()


def _desc(**over):
    """a descriptor that passes validation (the pointers are never dereferenced on the host); keys with a `cloud_` prefix go to the embedded
    s2m2_cloud_desc"""
    d = hip.VoxelDesc()
    c = d.cloud
    c.disp = c.occ = c.conf = c.image = 4096
    c.B, c.H, c.W, c.Hp, c.Wp, c.image_dtype = 1, 30, 50, 32, 64, 2
    c.fx, c.fy, c.cx, c.cy, c.baseline, c.doffs, c.depth_scale, c.depth_trunc, c.conf_min, c.occ_min = 1000.0, 1000.0, 25.0, 15.0, 100.0, 0.0, 1000.0, 3.0, 0.1, 0.5
    d.records = d.weights = d.count = d.index = d.stats = 8192
    d.workspace = 16384
    d.voxel_size, d.max_voxels, d.capacity = 0.05, 100, 100
    for k, v in over.items():
        setattr(c if k.startswith("cloud_") else d, k[6:] if k.startswith("cloud_") else k, v)
    return d


def test_symbols_version_and_header(lib):
    for name in ("s2m2_voxel", "s2m2_voxel_workspace_bytes", "s2m2_voxel_tile_rows", "s2m2_voxel_home_slot"):
        assert hasattr(lib, name) and name in hip.SIGNATURES
    assert lib.s2m2_version() == 800 and hip.ABI_VERSION == 800
    header = open(os.path.join(ROOT, "include", "s2m2_hip.h")).read()
    assert int(re.search(r"#define S2M2_ABI_VERSION (\d+)", header).group(1)) == 800
    assert "s2m2_voxel is NOT recorded" in header


@pytest.mark.parametrize("name,struct", [("s2m2_voxel_desc", hip.VoxelDesc)])
def test_desc_has_the_layout_of_the_header(tmp_path, name, struct):
    """every field: offset and size of the ctypes mirror against the struct compiled by gcc"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = [f[0] for f in struct._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "s2m2_hip.h"', "int main(void) {", f"  {name} d;",
             '  printf("%zu\\n", sizeof(d));']
    lines += [f'  printf("{n} %zu %zu\\n", offsetof({name}, {n}), sizeof(d.{n}));' for n in names]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == ctypes.sizeof(struct)
    for n, line in zip(names, out[1:]):
        field, off, size = line.split()
        f = getattr(struct, n)
        assert (field, int(off), int(size)) == (n, f.offset, f.size)
    assert names == ["cloud", "records", "weights", "count", "index", "stats", "workspace", "voxel_size", "max_voxels", "capacity"]
    assert struct.cloud.size == ctypes.sizeof(hip.CloudDesc)


def test_workspace_size_and_bad_arguments(lib):
    """64 bytes per slot, slots = the smallest power of two >= 2 * max_voxels, plus an int32 plane, the tile counts and the counters"""
    for B, H, W, mv in ((1, 1024, 1216, 1024 * 1216 // 4), (3, 48, 80, 100), (1, 1, 1, 1), (2, 3, 4100, 32), (1, 20, 30, 33)):
        slots = voxel_oracle.slots_of(mv)
        assert slots >= 2 * mv and slots & (slots - 1) == 0 and (slots == 2 or slots // 2 < 2 * mv) and hip.voxel_slots(mv) == slots
        n = lib.s2m2_voxel_workspace_bytes(B, H, W, mv)
        floor = B * (64 * slots + 4 * H * W)
        assert floor < n < floor + 4 * B * H + 4096 * B + 2048 and n % 16 == 0
        assert hip.voxel_workspace_bytes(B, H, W, mv) == n
    for B, H, W, mv in ((0, 4, 4, 8), (1, -1, 4, 8), (1, 4, 0, 8), (1, 1 << 16, 1 << 15, 8), (65536, 4, 4, 8), (1, 4, 4, 0), (1, 4, 4, -5),
                        (1, 4, 4, (1 << 29) + 1)):
        assert lib.s2m2_voxel_workspace_bytes(B, H, W, mv) == 0
    with pytest.raises(ValueError, match="bad extents"):
        hip.voxel_workspace_bytes(1, 0, 4, 8)
    with pytest.raises(ValueError, match="max_voxels"):
        hip.voxel_slots(0)


def test_tile_rows(lib):
    for H, W in ((1, 1), (500, 1), (37, 53), (1024, 1216), (10, 5000)):
        rows = lib.s2m2_voxel_tile_rows(H, W)
        assert 1 <= rows <= H and hip.voxel_tile_rows(H, W) == rows
    assert lib.s2m2_voxel_tile_rows(0, 5) == 0 and lib.s2m2_voxel_tile_rows(1 << 16, 1 << 15) == 0


def test_home_slot_is_a_function_into_the_table(lib):
    g = np.random.default_rng(0)
    cells = g.integers(-(1 << 20), 1 << 20, (2000, 3))
    for slots in (2, 64, 1 << 20, 1 << 30):
        home = [lib.s2m2_voxel_home_slot(int(a), int(b), int(c), slots) for a, b, c in cells[:300]]
        assert all(0 <= h < slots for h in home)
        assert home == [hip.voxel_home_slot(int(a), int(b), int(c), slots) for a, b, c in cells[:300]]
    # it spreads: 2000 random cells over 64 slots leave no slot empty and none with a tenth of them
    counts = np.bincount([lib.s2m2_voxel_home_slot(int(a), int(b), int(c), 64) for a, b, c in cells], minlength=64)
    assert counts.min() > 0 and counts.max() < 200
    # neighbouring cells do not share a home as a rule (a row of a plane is a run of neighbours)
    row = [lib.s2m2_voxel_home_slot(i, 7, 300, 1 << 16) for i in range(-50, 50)]
    assert len(set(row)) > 95
    assert lib.s2m2_voxel_home_slot(-(1 << 20), (1 << 20) - 1, 0, 64) >= 0
    for ix, iy, iz, slots in ((1 << 20, 0, 0, 64), (0, -(1 << 20) - 1, 0, 64), (0, 0, 1 << 20, 64), (0, 0, 0, 63), (0, 0, 0, 0), (0, 0, 0, 1),
                              (0, 0, 0, 1 << 31)):
        assert lib.s2m2_voxel_home_slot(ix, iy, iz, slots) == -1
    with pytest.raises(ValueError, match="bad arguments"):
        hip.voxel_home_slot(0, 0, 0, 100)


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
    # K23's own
    (dict(cloud_image=None), b"voxel: null pointer (image)"),
    (dict(voxel_size=0.0), b"voxel_size must be finite and > 0"),
    (dict(voxel_size=-0.05), b"voxel_size must be finite and > 0"),
    (dict(voxel_size=NAN), b"voxel_size must be finite and > 0"),
    (dict(voxel_size=INF), b"voxel_size must be finite and > 0"),
    (dict(voxel_size=1e-60), b"voxel_size must be finite and > 0"),
    (dict(voxel_size=1e60), b"voxel_size must be finite and > 0"),
    (dict(voxel_size=1e-44), b"too small"),
    (dict(max_voxels=0), b"max_voxels must be 1..2^29"),
    (dict(max_voxels=-3), b"max_voxels must be 1..2^29"),
    (dict(max_voxels=(1 << 29) + 1), b"max_voxels must be 1..2^29"),
    (dict(records=None, weights=None, count=None, index=None, stats=None, capacity=0), b"no output requested"),
    (dict(capacity=-1), b"negative capacity"),
    (dict(records=None, weights=None), b"null pointers (records and weights) with capacity 100"),
    (dict(records=8200), b"records must be 16-byte aligned"),
    (dict(workspace=None), b"null workspace"),
    (dict(workspace=16392), b"workspace must be 16-byte aligned"),
    (dict(weights=8193), b"must be 4-byte aligned"),
    (dict(count=8194), b"must be 4-byte aligned"),
    (dict(index=8195), b"must be 4-byte aligned"),
    (dict(stats=8197), b"must be 4-byte aligned"),
]


@pytest.mark.parametrize("over,msg", BAD, ids=[f"{'-'.join(o)}-{i}" for i, (o, _) in enumerate(BAD)])
def test_validation_fails_before_any_device_call(lib, over, msg):
    assert lib.s2m2_voxel(ctypes.byref(_desc(**over)), None) != 0
    assert msg in lib.s2m2_last_error(), lib.s2m2_last_error()
    assert lib.s2m2_last_error().startswith(b"voxel: ")


def test_what_is_allowed(lib):
    """records alone, weights alone, count alone with capacity 0, max_voxels = 2^29 and the ignored output fields of the embedded descriptor
    pass every check: the first failure is the one put there on purpose, which is tested last"""
    for over in (dict(weights=None), dict(records=None), dict(records=None, weights=None, index=None, stats=None, capacity=0),
                 dict(max_voxels=1 << 29), dict(cloud_capacity=-1, cloud_records=4104, cloud_count=4096, cloud_workspace=None)):
        assert lib.s2m2_voxel(ctypes.byref(_desc(workspace=None, **over)), None) != 0
        assert b"voxel: null workspace" in lib.s2m2_last_error(), lib.s2m2_last_error()


def test_null_descriptor(lib):
    assert lib.s2m2_voxel(None, None) != 0 and b"null descriptor" in lib.s2m2_last_error()


def test_refused_while_a_plan_records(lib):
    plan = ctypes.c_void_p()
    assert lib.s2m2_plan_begin(ctypes.byref(plan)) == 0
    try:
        assert lib.s2m2_voxel(ctypes.byref(_desc()), None) != 0
        assert b"not recorded in launch plans" in lib.s2m2_last_error()
        assert lib.s2m2_plan_launches(plan) == 0
    finally:
        lib.s2m2_plan_abort(plan)
        lib.s2m2_plan_destroy(plan)


def test_wrappers_reject_bad_operands(lib):
    import torch
    z = torch.zeros(1, 1, 32, 32)
    img = torch.zeros(1, 3, 32, 32, dtype=torch.uint8)
    kw = dict(fx=1.0, cx=0.0, cy=0.0, baseline=1.0)
    for bad, msg in ((dict(voxel_size=0.0), "voxel_size must be finite and > 0"), (dict(voxel_size=NAN), "voxel_size must be finite and > 0"),
                     (dict(voxel_size=INF), "voxel_size must be finite and > 0"), (dict(voxel_size=0.1, max_voxels=0), "max_voxels"),
                     (dict(voxel_size=0.1, max_voxels=2.5), "max_voxels"), (dict(voxel_size=0.1, max_voxels=(1 << 29) + 1), "max_voxels")):
        with pytest.raises(ValueError, match=msg):
            cloud.voxelize(z, z, z, img, **kw, **bad)
    with pytest.raises(ValueError, match="device tensors"):
        hip.voxel(z, z, z, img, fy=1.0, voxel_size=0.1, max_voxels=8, workspace=torch.zeros(1 << 16, dtype=torch.uint8),
                  count=torch.zeros(1, dtype=torch.int32), **kw)


# ---- the oracle against a dictionary

def _brute(disp, occ, conf, image, voxel_size, **cam):
    """the contract with Python integers: floor division and remainder for the cell and the offset, exact fractions for the colour"""
    c = cloud_oracle.cloud(disp, occ, conf, image, **cam)
    q = F(voxel_size) / F(1024.0)
    table, dropped, seen = {}, 0, []
    for i, pix in enumerate(c["index"].tolist()):
        with np.errstate(over="ignore", invalid="ignore"):
            r = [float(np.rint(F(a) / q)) for a in (c["x32"][i], c["y32"][i], c["z"][i])]
        if not all(abs(t) < 2.0 ** 30 for t in r):           # (false for NaN)
            dropped += 1
            continue
        X = [int(t) for t in r]
        seen.append(X)
        cell = tuple(math.floor(Fraction(t, 1024)) for t in X)
        e = table.setdefault(cell, dict(n=0, s=[0, 0, 0], c=[0, 0, 0], first=pix, pixels=[]))
        e["n"] += 1
        e["pixels"].append(pix)
        for k in range(3):
            e["s"][k] += X[k] - 1024 * cell[k]
            e["c"][k] += int(c["rgb"][i, k])
    ordered = sorted(table.items(), key=lambda kv: kv[1]["first"])
    rec = np.zeros((len(ordered), 4), np.int32)
    index = np.full(c["keep"].size, -1, np.int32)
    for r, (cell, e) in enumerate(ordered):
        assert all(0 <= s <= 1023 * e["n"] for s in e["s"])
        xyz = [F((cell[k] * 1024.0 + e["s"][k] / e["n"]) * float(q)) for k in range(3)]
        rgba = [math.floor(Fraction(e["c"][k], e["n"]) + Fraction(1, 2)) for k in range(3)] + [255]
        rec[r, :3] = np.array(xyz, F).view(np.int32)
        rec[r, 3] = np.frombuffer(bytes(rgba), "<i4")[0]
        index[e["pixels"]] = r
    return dict(records=rec, weights=np.array([e["n"] for _, e in ordered], np.int32), index=index.reshape(c["keep"].shape),
                stats=[len(c["index"]), dropped, 0, len(ordered)], cells=[cell for cell, _ in ordered], X=seen)


def _same(o, b):
    assert np.array_equal(o["records"], b["records"]) and np.array_equal(o["weights"], b["weights"])
    assert np.array_equal(o["index"], b["index"]) and o["stats"].tolist() == b["stats"]
    assert [tuple(v) for v in o["voxels"].tolist()] == b["cells"]


def _scene(H, W, z, image=None, keep=None):
    """maps whose kept pixels have depth z (H,W) exactly: fx = baseline = depth_scale = 1, so z = 1 / d with d = 1 / z a power of two here"""
    z = np.broadcast_to(np.asarray(z, dtype=F), (H, W))
    disp = (F(1.0) / z).astype(F)
    conf = np.ones((H, W), F) if keep is None else np.asarray(keep, dtype=F)
    img = np.zeros((3, H, W), np.uint8) if image is None else image
    return disp, np.ones((H, W), F), conf, img


def test_negative_coordinates_exact_multiples_and_minus_one():
    """q = 1 (voxel_size 1024), fx = 1, z = 1: X = u - cx, Y = v - cy.  cx = 2, cy = 1 give X = -2, -1, 0, ... and Y = -1, 0, ...; z = 512
    gives the multiples of 512, and so X = -1024, 0, 1024 among them"""
    cam = dict(fx=1.0, fy=1.0, cx=2.0, cy=1.0, baseline=1.0, depth_scale=1.0, depth_trunc=4096.0)
    H, W = 3, 7
    for z in (1.0, 512.0):
        s = _scene(H, W, z)
        o, b = voxel_oracle.voxelize(*s, voxel_size=1024.0, **cam), _brute(*s, 1024.0, **cam)
        _same(o, b)
        xs = {x[0] for x in b["X"]}
        assert (xs >= {-2, -1, 0, 1}) if z == 1.0 else (xs >= {-1024, 0, 1024})
    # X = -1 lies in cell -1 at offset 1023, X = -1024 in cell -1 at offset 0, X = 1024 in cell 1 at offset 0: the centroid of a single point
    # is the point
    s = _scene(1, 7, 1.0)
    o = voxel_oracle.voxelize(*s, voxel_size=1024.0, **{**cam, "cy": 0.0})
    assert o["voxels"][:, 0].tolist() == [-1, 0] and o["weights"].tolist() == [2, 5]
    assert o["records"][:, :3].view(F)[:, 0].tolist() == [-1.5, 2.0]
    s = _scene(1, 5, 512.0)
    o = voxel_oracle.voxelize(*s, voxel_size=1024.0, **{**cam, "cy": 0.0})
    assert o["voxels"][:, 0].tolist() == [-1, 0, 1] and o["weights"].tolist() == [2, 2, 1]        # X = -1024, -512 | 0, 512 | 1024
    assert o["records"][:, :3].view(F)[:, 0].tolist() == [-768.0, 256.0, 1024.0]


def test_colour_rounding_ties_go_up():
    cam = dict(fx=1.0, fy=1.0, cx=-1.0, cy=-1.0, baseline=1.0, depth_scale=1.0, depth_trunc=4096.0)
    img = np.zeros((3, 1, 4), np.uint8)
    img[0, 0] = [1, 2, 2, 1]            # mean 1.5 -> 2
    img[1, 0] = [0, 0, 0, 1]            # mean 0.25 -> 0
    img[2, 0] = [255, 254, 255, 254]    # mean 254.5 -> 255
    s = _scene(1, 4, 1.0, img)
    o, b = voxel_oracle.voxelize(*s, voxel_size=1024.0, **cam), _brute(*s, 1024.0, **cam)
    _same(o, b)
    assert o["weights"].tolist() == [4] and o["records"][0, 3:].view(np.uint8).tolist() == [2, 0, 255, 255]


def test_out_of_range_rule():
    """z = 2^20 and q = 1: X = u * 2^20.  u = 1023 is the last column in range (1023 * 2^20 < 2^30), u = 1024 gives exactly 2^30 and is
    dropped; d <= 0 with depth_trunc None sits at z = 1e9 and is dropped by its Z"""
    cam = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, baseline=1.0, depth_scale=1.0, depth_trunc=2.0 ** 21)
    s = _scene(1, 1026, 2.0 ** 20)
    o, b = voxel_oracle.voxelize(*s, voxel_size=1024.0, **cam), _brute(*s, 1024.0, **cam)
    _same(o, b)
    assert o["stats"].tolist() == [1026, 2, 0, 1024] and o["index"][0, 1023] == 1023 and o["index"][0, 1024] == -1
    assert o["voxels"][-1].tolist() == [1023 * 1024, 0, 1024]
    disp, occ, conf, img = _scene(2, 5, 1.0)
    disp[0, 1], disp[1, 3] = 0.0, -2.0
    cam = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, baseline=1000.0, depth_scale=1000.0, depth_trunc=None)     # z = 1 at d = 1, 1e6 at d <= 0
    o, b = voxel_oracle.voxelize(disp, occ, conf, img, voxel_size=0.5, **cam), _brute(disp, occ, conf, img, 0.5, **cam)     # Z = 1e6 * 2048
    _same(o, b)
    assert o["stats"].tolist() == [10, 2, 0, 8] and o["index"][0, 1] == -1 and o["index"][1, 3] == -1


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_against_the_dictionary_on_a_random_scene(seed):
    g = np.random.default_rng(seed)
    H, W = 13, 17
    k = cloud.read_calib_file(CALIB)
    cam = dict(fx=float(k["cam0"][0, 0]), fy=float(k["cam0"][1, 1]), cx=8.0, cy=6.0, baseline=float(k["baseline"]), doffs=float(k["doffs"]),
               depth_trunc=None if seed == 2 else 30.0)
    disp = (g.random((H, W), dtype=F) * F(60.0) + F(40.0)).astype(F)
    disp[g.random((H, W)) < 0.1] = -1.0
    conf, occ = g.random((H, W), dtype=F), g.random((H, W), dtype=F) * F(0.5) + F(0.5)
    img = g.integers(0, 256, (3, H, W), dtype=np.uint8)
    for vs in (0.004, 0.05, 1.0):
        o, b = voxel_oracle.voxelize(disp, occ, conf, img, voxel_size=vs, **cam), _brute(disp, occ, conf, img, vs, **cam)
        _same(o, b)
        assert 0 < o["stats"][3] <= o["stats"][0] - o["stats"][1] and int(o["weights"].sum()) == o["stats"][0] - o["stats"][1]
    assert o["stats"][3] < o["stats"][0] // 2                   # the coarse grid merges points


# ---- the runner's option rules (usage errors, before the engine is loaded: no GPU needed)

def test_runner_option_rules(lib):
    from s2m2_amd.build import RUNNER
    base = [RUNNER, "absent.s2m2", "l.f32", "r.f32"]
    for extra, msg in ((["--calib", CALIB, "--voxel", "0.05"], "--voxel and --voxel-ply come together"),
                       (["--calib", CALIB, "--voxel-ply", "v.ply"], "--voxel and --voxel-ply come together"),
                       (["--voxel", "0.05", "--voxel-ply", "v.ply"], "--voxel needs --calib"),
                       (["--calib", CALIB, "--ply", "x.ply", "--voxel-max", "100"], "--voxel-max needs --voxel"),
                       (["--calib", CALIB, "--voxel", "0", "--voxel-ply", "v.ply"], "--voxel: a number > 0"),
                       (["--calib", CALIB, "--voxel", "-1", "--voxel-ply", "v.ply"], "--voxel: a number > 0"),
                       (["--calib", CALIB, "--voxel", "nan", "--voxel-ply", "v.ply"], "--voxel: a number > 0"),
                       (["--calib", CALIB, "--voxel", "inf", "--voxel-ply", "v.ply"], "--voxel: a number > 0"),
                       (["--calib", CALIB, "--voxel", "5cm", "--voxel-ply", "v.ply"], "--voxel: a number > 0"),
                       (["--calib", CALIB, "--voxel", "0.05", "--voxel-ply", "v.ply", "--voxel-max", "0"], "--voxel-max: an integer >= 1"),
                       (["--calib", CALIB, "--voxel", "0.05", "--voxel-ply", "v.ply", "--voxel-max", "many"], "--voxel-max: an integer >= 1"),
                       (["--calib", CALIB, "--voxel", "0.05", "--voxel-ply", "v.ply", "--depth", "d.f32"], "--depth needs --ply or --mesh"),
                       (["--calib", CALIB], "--calib and --ply come together")):
        p = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and msg in p.stderr, (extra, p.stderr)
    # complete without --ply / --mesh, with them, and behind --min-size: the next failure is the missing engine
    for extra in (["--voxel", "0.05", "--voxel-ply", "v.ply"], ["--voxel", "0.05", "--voxel-ply", "v.ply", "--voxel-max", "5000", "--ply", "x.ply"],
                  ["--voxel", "1e-3", "--voxel-ply", "v.ply", "--mesh", "m.ply", "--min-size", "5"]):
        p = subprocess.run(base + ["--calib", CALIB] + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and "engine_load: cannot open" in p.stderr, p.stderr
