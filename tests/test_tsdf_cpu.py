"""CPU-side checks of K24 (include/s2m2_hip.h: s2m2_tsdf_integrate, s2m2_tsdf_extract; s2m2_amd/cloud.py: TsdfVolume): the numpy oracle the GPU
tests compare against, checked against a scalar per-voxel loop and against scenes whose surface is known; the colour recurrence's bounds; the
boundary (symbols, descriptor layouts, workspace size, every validation path -- all of which return before any device call, there is no GPU
here); the wrappers' own errors; the runner's LIST and option rules."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cloud_oracle
import tsdf_oracle as O
import tsdf_scenes as S
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


# ---- the oracle against a scalar loop

def _scalar_integrate(vol, disp, occ, conf, image, poses, *, origin, voxel_size, trunc, max_weight, carve, fx, fy, cx, cy, **cam):
    """the header's formulas voxel by voxel with numpy float32 SCALARS (every operation rounds once) and Python integers"""
    B, _, H, W = image.shape
    Nz, Ny, Nx, _ = vol.shape
    out = vol.copy()
    pairs = [cloud_oracle.cloud(cloud_oracle.crop(disp[b], H, W), cloud_oracle.crop(occ[b], H, W), cloud_oracle.crop(conf[b], H, W), image[b],
                                fx=fx, fy=fy, cx=cx, cy=cy, **cam) for b in range(B)]
    o, vs, tr = [F(a) for a in origin], F(voxel_size), F(trunc)
    for k in range(Nz):
        for j in range(Ny):
            for i in range(Nx):
                w = out[k, j, i].view(np.uint32)
                tsdf, weight = w[:1].view(F)[0], int(w[1:2].view(np.int32)[0])
                col, pad, touched = [int(w[2]) & 0xffff, int(w[2]) >> 16, int(w[3]) & 0xffff], int(w[3]) >> 16, False
                x, y, z = o[0] + F(i) * vs, o[1] + F(j) * vs, o[2] + F(k) * vs
                for b in range(B):
                    q = [F(a) for a in poses[b]]
                    X = ((q[0] * x + q[1] * y) + q[2] * z) + q[3]
                    Y = ((q[4] * x + q[5] * y) + q[6] * z) + q[7]
                    Z = ((q[8] * x + q[9] * y) + q[10] * z) + q[11]
                    if not (Z > 0 and np.isfinite(Z)):
                        continue
                    fu, fv = np.rint((F(fx) * X) / Z + F(cx)), np.rint((F(fy) * Y) / Z + F(cy))
                    if not (fu >= 0 and fu < W and fv >= 0 and fv < H):
                        continue
                    u, v = int(fu), int(fv)
                    if not pairs[b]["keep"][v, u]:
                        continue
                    sdf = pairs[b]["depth"][v, u] - Z
                    if not sdf >= -tr or (not carve and sdf > tr):
                        continue
                    d = min(sdf / tr, F(1.0))
                    Wf = F(weight)
                    tsdf = (tsdf * Wf + d) / (Wf + F(1.0))
                    rgb = cloud_oracle.colour_bytes(image[b])[:, v, u]
                    col = [(c * weight + (int(byte) << 8) + ((weight + 1) >> 1)) // (weight + 1) for c, byte in zip(col, rgb)]
                    weight = min(weight + 1, max_weight)
                    touched = True
                if touched:
                    w[0], w[1] = np.array([tsdf], F).view(np.uint32)[0], weight
                    w[2], w[3] = col[0] | (col[1] << 16), col[2] | (pad << 16)
    return out


@pytest.mark.parametrize("carve", [False, True])
def test_oracle_against_a_scalar_loop(carve):
    grid = dict(dims=(7, 5, 6), origin=(-0.3, -0.25, 1.75), voxel_size=0.1, trunc=0.2)
    frames = S.frames(["steps", "plane", "tilt"])
    poses = np.array([S.IDENTITY, S.rot_xy(0.1, -0.15, (0.05, -0.03, 0.1)), [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -1.9]], F)
    kw = dict(origin=grid["origin"], voxel_size=grid["voxel_size"], trunc=grid["trunc"], max_weight=2, carve=carve, **S.CAM)
    start = O.empty(grid["dims"])
    start[..., 3] = 0x7abc0000                        # the pad travels
    a, diag = O.integrate(start, *frames, poses, **kw)
    b = _scalar_integrate(start, *frames, poses, **kw)
    assert a.tobytes() == b.tobytes()
    seen = {int(c) for d in diag for c in np.unique(d["cls"])}
    assert seen >= {O.BEHIND, O.BELOW_BAND, O.UPDATED} and (O.IN_FRONT in seen) != carve
    assert (O.unpack(a)["weight"] == 2).any() and (O.unpack(a)["pad"] == 0x7abc).all()


def test_the_prototype_scene_of_the_issue():
    """a plane at z = 2, a 19x13x11 grid, vs 0.1, trunc 0.3, 3 frames, max_weight 2: every surface point lies at z = 2.0 exactly and on a z
    edge; carving updates more voxels than the band alone"""
    grid = S.GRID_A
    frames = S.frames(["plane"] * 3, holes=False)
    kw = dict(origin=grid["origin"], voxel_size=grid["voxel_size"], trunc=grid["trunc"], max_weight=2, **S.CAM)
    counts = {}
    for carve in (False, True):
        vol, diag = O.integrate(O.empty(grid["dims"]), *frames, np.array([S.IDENTITY] * 3, F), carve=carve, **kw)
        counts[carve] = int((O.unpack(vol)["weight"] > 0).sum())
        e = O.extract(vol, origin=grid["origin"], voxel_size=grid["voxel_size"])
        assert e["count"] > 100 and (e["axis"] == 2).all()
        assert (np.abs(e["records"][:, 2].view(F) - F(2.0)) <= 2e-6).all()
        assert (O.unpack(vol)["weight"][O.unpack(vol)["weight"] > 0] == 2).all()
    assert 0 < counts[False] < counts[True]


def test_a_sphere_is_recovered_within_one_voxel():
    """depth of a sphere of radius 0.5 at (0, 0, 2.2) in front of a wall at z = 3: every extracted point lies within one voxel of it"""
    v, u = np.mgrid[0:S.H, 0:S.W]
    dx, dy = (u - S.CAM["cx"]) / S.CAM["fx"], (v - S.CAM["cy"]) / S.CAM["fy"]
    a, bq, c = dx * dx + dy * dy + 1.0, -2.0 * 2.2, 2.2 * 2.2 - 0.25
    disc = bq * bq - 4 * a * c
    z = np.where(disc > 0, (-bq - np.sqrt(np.maximum(disc, 0))) / (2 * a), 3.0)
    disp = (1.0 / z).astype(F)[None]
    one = np.ones_like(disp)
    img = np.full((1, 3, S.H, S.W), 200, np.uint8)
    vs = 0.05
    dims, origin = (25, 25, 21), (-0.6, -0.6, 1.5)
    vol, _ = O.integrate(O.empty(dims), disp, one, one, img, np.array([S.IDENTITY], F), origin=origin, voxel_size=vs, trunc=4 * vs, max_weight=64,
                         **S.CAM)
    e = O.extract(vol, origin=origin, voxel_size=vs)
    p = e["records"][:, :3].view(F).astype(np.float64)
    r = np.linalg.norm(p - np.array([0.0, 0.0, 2.2]), axis=1)
    assert e["count"] > 200 and (np.abs(r - 0.5) < vs).all()
    g = e["gradients"].astype(np.float64)
    outward = (g * (p - np.array([0.0, 0.0, 2.2]))).sum(1)
    assert (outward > 0).mean() > 0.95                   # the gradient points from the surface to free space
    assert (e["records"][:, 3].view(np.uint32) == 0xffc8c8c8).all()


def test_colour_recurrence_bounds():
    """the 8.8 colour never leaves 0 .. 65280 and the numerator stays below 2^32 at the largest weight"""
    worst = 65280 * 32767 + (255 << 8) + (32768 >> 1)
    assert worst < 1 << 32
    for byte in (0, 1, 128, 255):
        c = 65280
        for w in (0, 1, 2, 100, 32766, 32767):
            n = (c * w + (byte << 8) + ((w + 1) >> 1)) // (w + 1)
            assert 0 <= n <= 65280
    c, w = 0, 0                                        # converges to the byte and stays there
    for _ in range(300):
        c = (c * w + (255 << 8) + ((w + 1) >> 1)) // (w + 1)
        w = min(w + 1, 32767)
    assert c == 65280


def test_an_all_zero_volume_is_empty():
    e = O.extract(O.empty((5, 4, 3)), origin=(0, 0, 0), voxel_size=1.0)
    assert e["count"] == 0 and e["records"].shape == (0, 4) and not e["observed"].any()


# ---- the boundary

def _desc(**over):
    """an integrate descriptor that passes validation (the pointers are never dereferenced on the host); keys with a `cloud_` prefix go to the
    embedded s2m2_cloud_desc"""
    d = hip.TsdfDesc()
    c = d.cloud
    c.disp = c.occ = c.conf = c.image = 4096
    c.B, c.H, c.W, c.Hp, c.Wp, c.image_dtype = 2, 30, 50, 32, 64, 2
    c.fx, c.fy, c.cx, c.cy, c.baseline, c.doffs, c.depth_scale, c.depth_trunc, c.conf_min, c.occ_min = 1000.0, 1000.0, 25.0, 15.0, 100.0, 0.0, 1000.0, 3.0, 0.1, 0.5
    d.volume, d.poses = 1 << 20, 8192
    d.Nx, d.Ny, d.Nz, d.max_weight, d.carve = 19, 13, 11, 64, 0
    d.origin = (ctypes.c_double * 3)(-1.0, -1.0, 0.5)
    d.voxel_size, d.trunc = 0.05, 0.2
    for k, v in over.items():
        if k.startswith("origin"):
            d.origin[int(k[6:])] = v
        else:
            setattr(c if k.startswith("cloud_") else d, k[6:] if k.startswith("cloud_") else k, v)
    return d


def _xdesc(**over):
    d = hip.TsdfExtractDesc()
    d.volume, d.records, d.gradients, d.count, d.workspace = 1 << 20, 1 << 21, 1 << 22, 8192, 16384
    d.Nx, d.Ny, d.Nz, d.min_weight, d.capacity = 19, 13, 11, 1, 100
    d.origin = (ctypes.c_double * 3)(-1.0, -1.0, 0.5)
    d.voxel_size = 0.05
    for k, v in over.items():
        if k.startswith("origin"):
            d.origin[int(k[6:])] = v
        else:
            setattr(d, k, v)
    return d


def test_symbols_version_and_header(lib):
    for name in ("s2m2_tsdf_integrate", "s2m2_tsdf_extract", "s2m2_tsdf_workspace_bytes", "s2m2_tsdf_tile_voxels"):
        assert hasattr(lib, name) and name in hip.SIGNATURES
    assert lib.s2m2_version() == 800 and hip.ABI_VERSION == 800
    header = open(os.path.join(ROOT, "include", "s2m2_hip.h")).read()
    assert int(re.search(r"#define S2M2_ABI_VERSION (\d+)", header).group(1)) == 800
    assert "s2m2_tsdf_integrate and s2m2_tsdf_extract are NOT recorded" in header


@pytest.mark.parametrize("name,struct,fields", [
    ("s2m2_tsdf_desc", hip.TsdfDesc, ["cloud", "volume", "poses", "Nx", "Ny", "Nz", "max_weight", "carve", "origin", "voxel_size", "trunc"]),
    ("s2m2_tsdf_extract_desc", hip.TsdfExtractDesc,
     ["volume", "records", "gradients", "count", "workspace", "Nx", "Ny", "Nz", "min_weight", "capacity", "origin", "voxel_size"])])
def test_descs_have_the_layout_of_the_header(tmp_path, name, struct, fields):
    """every field: offset and size of the ctypes mirror against the struct compiled by gcc"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = [f[0] for f in struct._fields_]
    assert names == fields
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


def test_workspace_tile_and_bad_dims(lib):
    for dims in ((19, 13, 11), (1, 1, 1), (512, 512, 512), (1, 1, (1 << 29) - 1), (37, 21, 23)):
        tile = lib.s2m2_tsdf_tile_voxels(*dims)
        n = lib.s2m2_tsdf_workspace_bytes(*dims)
        tiles = -(-dims[0] * dims[1] * dims[2] // tile)
        assert tile >= 256 and tile % 256 == 0 and 4 * tiles <= n < 4 * tiles + 256 and n % 256 == 0
        assert hip.tsdf_tile_voxels(*dims) == tile and hip.tsdf_workspace_bytes(*dims) == n
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (1024, 1024, 512), (1 << 15, 1 << 15, 1), (1 << 30, 1, 1)):
        assert lib.s2m2_tsdf_workspace_bytes(*dims) == 0 and lib.s2m2_tsdf_tile_voxels(*dims) == 0
    with pytest.raises(ValueError, match="bad extents"):
        hip.tsdf_workspace_bytes(0, 4, 4)


BAD = [
    # the input side of s2m2_cloud
    (dict(cloud_disp=None), b"null pointer"),
    (dict(cloud_occ=None), b"null pointer"),
    (dict(cloud_conf=None), b"null pointer"),
    (dict(cloud_H=33), b"larger than the maps"),
    (dict(cloud_W=65), b"larger than the maps"),
    (dict(cloud_B=0), b"non-positive extents"),
    (dict(cloud_H=0), b"non-positive extents"),
    (dict(cloud_Wp=0), b"non-positive extents"),
    (dict(cloud_fx=0.0), b"fx and fy must be positive"),
    (dict(cloud_fy=-1.0), b"fx and fy must be positive"),
    (dict(cloud_depth_scale=0.0), b"depth_scale must be positive"),
    (dict(cloud_image_dtype=3), b"unsupported image dtype"),
    (dict(cloud_disp=4098), b"4-byte aligned"),
    (dict(cloud_H=1 << 16, cloud_W=1 << 15, cloud_Hp=1 << 16, cloud_Wp=1 << 15), b"extents too large"),
    # K24's own
    (dict(cloud_image=None), b"null pointer (image)"),
    (dict(volume=None), b"null pointer (volume)"),
    (dict(poses=None), b"null pointer (poses)"),
    (dict(volume=(1 << 20) + 8), b"volume must be 16-byte aligned"),
    (dict(poses=8194), b"poses must be 4-byte aligned"),
    (dict(Nx=0), b"non-positive dims"),
    (dict(Ny=-2), b"non-positive dims"),
    (dict(Nz=0), b"non-positive dims"),
    (dict(Nx=1024, Ny=1024, Nz=512), b"dims too large"),
    (dict(Nx=1 << 20, Ny=1 << 20, Nz=1 << 20), b"dims too large"),
    (dict(voxel_size=0.0), b"voxel_size must be finite and > 0"),
    (dict(voxel_size=-0.05), b"voxel_size must be finite and > 0"),
    (dict(voxel_size=NAN), b"voxel_size must be finite and > 0"),
    (dict(voxel_size=INF), b"voxel_size must be finite and > 0"),
    (dict(voxel_size=1e-60), b"voxel_size must be finite and > 0"),
    (dict(voxel_size=1e60), b"voxel_size must be finite and > 0"),
    (dict(trunc=0.0), b"trunc must be finite and > 0"),
    (dict(trunc=-1.0), b"trunc must be finite and > 0"),
    (dict(trunc=NAN), b"trunc must be finite and > 0"),
    (dict(trunc=INF), b"trunc must be finite and > 0"),
    (dict(trunc=1e-60), b"trunc must be finite and > 0"),
    (dict(origin0=NAN), b"origin must be finite"),
    (dict(origin1=INF), b"origin must be finite"),
    (dict(origin2=1e60), b"origin must be finite"),
    (dict(max_weight=0), b"max_weight must be 1..32767"),
    (dict(max_weight=-1), b"max_weight must be 1..32767"),
    (dict(max_weight=32768), b"max_weight must be 1..32767"),
]


@pytest.mark.parametrize("over,msg", BAD, ids=[f"{'-'.join(o)}-{i}" for i, (o, _) in enumerate(BAD)])
def test_integrate_validation_fails_before_any_device_call(lib, over, msg):
    assert lib.s2m2_tsdf_integrate(ctypes.byref(_desc(**over)), None) != 0
    assert msg in lib.s2m2_last_error(), lib.s2m2_last_error()
    assert lib.s2m2_last_error().startswith(b"tsdf_integrate: ")


XBAD = [
    (dict(volume=None), b"null pointer (volume)"),
    (dict(volume=(1 << 20) + 4), b"volume must be 16-byte aligned"),
    (dict(Nx=0), b"non-positive dims"),
    (dict(Nx=1024, Ny=1024, Nz=512), b"dims too large"),
    (dict(voxel_size=0.0), b"voxel_size must be finite and > 0"),
    (dict(voxel_size=NAN), b"voxel_size must be finite and > 0"),
    (dict(origin1=NAN), b"origin must be finite"),
    (dict(min_weight=0), b"min_weight must be >= 1"),
    (dict(min_weight=-3), b"min_weight must be >= 1"),
    (dict(records=None, gradients=None, count=None, capacity=0), b"no output requested"),
    (dict(capacity=-1), b"negative capacity"),
    (dict(records=None, gradients=None), b"null pointers (records and gradients) with capacity 100"),
    (dict(records=(1 << 21) + 8), b"records must be 16-byte aligned"),
    (dict(gradients=(1 << 22) + 2), b"must be 4-byte aligned"),
    (dict(count=8193), b"must be 4-byte aligned"),
    (dict(workspace=None), b"null workspace"),
    (dict(workspace=16386), b"workspace must be 4-byte aligned"),
]


@pytest.mark.parametrize("over,msg", XBAD, ids=[f"{'-'.join(o)}-{i}" for i, (o, _) in enumerate(XBAD)])
def test_extract_validation_fails_before_any_device_call(lib, over, msg):
    assert lib.s2m2_tsdf_extract(ctypes.byref(_xdesc(**over)), None) != 0
    assert msg in lib.s2m2_last_error(), lib.s2m2_last_error()
    assert lib.s2m2_last_error().startswith(b"tsdf_extract: ")


def test_what_is_allowed(lib):
    """the ignored output fields of the embedded descriptor, max_weight at both ends, records alone, gradients alone and the count alone pass
    every check: the first failure is the one put there on purpose, which is tested last"""
    for over in (dict(cloud_capacity=-1, cloud_records=4104, cloud_count=4096, cloud_workspace=None), dict(max_weight=1), dict(max_weight=32767),
                 dict(carve=7)):
        assert lib.s2m2_tsdf_integrate(ctypes.byref(_desc(poses=8194, **over)), None) != 0
        assert b"poses must be 4-byte aligned" in lib.s2m2_last_error(), lib.s2m2_last_error()
    for over in (dict(gradients=None), dict(records=None), dict(records=None, gradients=None, capacity=0), dict(count=None)):
        assert lib.s2m2_tsdf_extract(ctypes.byref(_xdesc(workspace=None, **over)), None) != 0
        assert b"tsdf_extract: null workspace" in lib.s2m2_last_error(), lib.s2m2_last_error()


def test_null_descriptors(lib):
    assert lib.s2m2_tsdf_integrate(None, None) != 0 and b"null descriptor" in lib.s2m2_last_error()
    assert lib.s2m2_tsdf_extract(None, None) != 0 and b"null descriptor" in lib.s2m2_last_error()


def test_refused_while_a_plan_records(lib):
    plan = ctypes.c_void_p()
    assert lib.s2m2_plan_begin(ctypes.byref(plan)) == 0
    try:
        assert lib.s2m2_tsdf_integrate(ctypes.byref(_desc()), None) != 0
        assert b"not recorded in launch plans" in lib.s2m2_last_error()
        assert lib.s2m2_tsdf_extract(ctypes.byref(_xdesc()), None) != 0
        assert b"not recorded in launch plans" in lib.s2m2_last_error()
        assert lib.s2m2_plan_launches(plan) == 0
    finally:
        lib.s2m2_plan_abort(plan)
        lib.s2m2_plan_destroy(plan)


def test_wrappers_reject_bad_operands(lib):
    import torch
    for bad, msg in ((dict(dims=(0, 4, 4), voxel_size=0.1), "bad dims"), (dict(dims=(1024, 1024, 512), voxel_size=0.1), "bad dims"),
                     (dict(dims=(4, 4, 4), voxel_size=0.0), "voxel_size must be finite and > 0"),
                     (dict(dims=(4, 4, 4), voxel_size=NAN), "voxel_size must be finite and > 0"),
                     (dict(dims=(4, 4, 4), voxel_size=0.1, trunc=-1.0), "trunc must be finite and > 0"),
                     (dict(dims=(4, 4, 4), voxel_size=0.1, max_weight=0), "max_weight"),
                     (dict(dims=(4, 4, 4), voxel_size=0.1, max_weight=40000), "max_weight"),
                     (dict(dims=(4, 4, 4), voxel_size=0.1, origin=(0.0, NAN, 0.0)), "origin")):
        with pytest.raises(ValueError, match=msg):
            cloud.TsdfVolume(**{"origin": (0.0, 0.0, 0.0), "device": "cpu", **bad})
    tv = cloud.TsdfVolume((4, 5, 6), 0.1, (0.0, 0.0, 1.0), device="cpu")
    assert tv.trunc == pytest.approx(0.4) and tuple(tv.buffer.shape) == (6, 5, 4, 4) and not tv.buffer.any()
    assert tuple(tv.tsdf().shape) == (6, 5, 4) and tuple(tv.weight().shape) == (6, 5, 4) and tuple(tv.colour().shape) == (6, 5, 4, 3)
    z = torch.zeros(2, 1, 32, 32)
    img = torch.zeros(2, 3, 32, 32, dtype=torch.uint8)
    kw = dict(fx=1.0, cx=0.0, cy=0.0, baseline=1.0)
    with pytest.raises(ValueError, match=r"R is \(3,3\) or \(2,3,3\)"):
        tv.integrate(z, z, z, img, R=np.eye(4), t=np.zeros(3), **kw)
    with pytest.raises(ValueError, match=r"t is \(3,\) or \(2,3\)"):
        tv.integrate(z, z, z, img, R=np.eye(3), t=np.zeros((3, 3)), **kw)
    with pytest.raises(ValueError, match="device tensors"):
        tv.integrate(z, z, z, img, R=np.eye(3), t=np.zeros(3), **kw)
    with pytest.raises(ValueError, match="negative capacity"):
        tv.extract(capacity=-1)
    vol = torch.zeros(6, 5, 4, 4, dtype=torch.int32)
    ws = torch.zeros(256, dtype=torch.uint8)
    with pytest.raises(ValueError, match="device tensors"):
        hip.tsdf_extract(vol, origin=(0, 0, 0), voxel_size=0.1, workspace=ws, count=torch.zeros(1, dtype=torch.int32))


# ---- the runner's LIST and option rules (usage errors, before the engine is loaded: no GPU needed)

def test_runner_tsdf_rules(lib, tmp_path):
    from s2m2_amd.build import RUNNER
    good = tmp_path / "list.txt"
    good.write_text("# two frames\n\nl0.f32 r0.f32 i0.u8 1 0 0 0 0 1 0 0 0 0 1 0\n  l1.f32 r1.f32 i1.u8 1 0 0 0.5 0 1 0 -0.25 0 0 1 1e-1  \n")
    full = ["--tsdf-frames", str(good), "--tsdf-dims", "19,13,11", "--tsdf-voxel", "0.1", "--tsdf-origin", "-0.9,-0.6,1.5", "--calib", CALIB,
            "--tsdf-ply", "t.ply"]

    def run(args):
        p = subprocess.run([RUNNER] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert p.returncode != 0 and p.stderr.startswith("s2m2_run_engine: ") and p.stderr.count("\n") == 1, p.stderr
        return p.stderr

    def swap(flag, value):
        a = list(full)
        a[a.index(flag) + 1] = value
        return a

    def drop(flag):
        a = list(full)
        i = a.index(flag)
        return a[:i] + a[i + 2:]

    # complete: the next failure is the missing engine; also with every optional flag
    assert "engine_load: cannot open" in run(["absent.s2m2"] + full)
    assert "engine_load: cannot open" in run(["absent.s2m2"] + full + ["--tsdf-trunc", "0.3", "--tsdf-min-weight", "2", "--tsdf-carve", "--unfiltered",
                                                                       "--depth-trunc", "10", "--conf-min", "0.2"])
    assert "takes ENGINE alone" in run(["absent.s2m2", "l.f32", "r.f32"] + full)
    assert "need --tsdf-frames" in run(["absent.s2m2"] + drop("--tsdf-frames"))
    for flag in ("--tsdf-dims", "--tsdf-voxel", "--tsdf-origin", "--calib", "--tsdf-ply"):
        assert "--tsdf-frames needs --tsdf-dims, --tsdf-voxel, --tsdf-origin, --calib and --tsdf-ply" in run(["absent.s2m2"] + drop(flag))
    for extra in (["--ply", "x.ply"], ["--repeat", "3"], ["--voxel", "0.1", "--voxel-ply", "v.ply"], ["--out", "."], ["--min-size", "5"]):
        assert "comes without the options of a single pair" in run(["absent.s2m2"] + full + extra)
    for bad in ("19,13", "19,13,11,2", "19,13,0", "19,x,11", "1.5,2,3", "1024,1024,512", "-1,2,3", "19,13,11 "):
        assert "--tsdf-dims: three integers >= 1" in run(["absent.s2m2"] + swap("--tsdf-dims", bad))
    for bad in ("0", "-0.1", "nan", "inf", "5cm"):
        assert "--tsdf-voxel: a number > 0" in run(["absent.s2m2"] + swap("--tsdf-voxel", bad))
        assert "--tsdf-trunc: a number > 0" in run(["absent.s2m2"] + full + ["--tsdf-trunc", bad])
    for bad in ("0,0", "0,0,nan", "a,b,c", "0,0,0,0"):
        assert "--tsdf-origin: three finite numbers" in run(["absent.s2m2"] + swap("--tsdf-origin", bad))
    for bad in ("0", "-2", "two", "40000"):
        assert "--tsdf-min-weight: an integer in 1..32767" in run(["absent.s2m2"] + full + ["--tsdf-min-weight", bad])
    # LIST itself
    assert "cannot open the file" in run(["absent.s2m2"] + swap("--tsdf-frames", "nowhere.txt"))
    for text, msg in (("", "no frame"), ("# nothing\n\n", "no frame"), ("l.f32 r.f32 i.u8 1 0 0 0 0 1 0 0 0 0 1\n", "line 1: "),
                      ("l.f32 r.f32 i.u8 1 0 0 0 0 1 0 0 0 0 1 0 7\n", "line 1: "), ("l.f32 r.f32 1 0 0 0 0 1 0 0 0 0 1 0\n", "line 1: "),
                      ("# head\nl.f32 r.f32 i.u8 1 0 0 0 0 1 0 0 0 0 1 0\nl.f32 r.f32 i.u8 1 0 0 0 0 1 0 0 0 0 nan 0\n", "line 3: ")):
        (tmp_path / "bad.txt").write_text(text)
        assert msg in run(["absent.s2m2"] + swap("--tsdf-frames", str(tmp_path / "bad.txt")))
    # without these flags the program behaves as before
    assert "engine_load: cannot open" in run(["absent.s2m2", "l.f32", "r.f32"])
