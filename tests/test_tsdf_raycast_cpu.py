"""CPU-side checks of K26 (include/s2m2_hip.h: s2m2_tsdf_raycast; s2m2_amd/cloud.py: TsdfVolume.raycast): the numpy oracle the GPU tests compare
against (against a plain scalar transcription of the rule, and on the dyadic plane, where the answer is known exactly), and the boundary:
symbols, descriptor layout, every validation path of the entry point -- all of which return before any device call, there is no GPU here --,
the wrappers' own errors, raised before any library call, and the runner's option rules."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import tsdf_oracle as O
import tsdf_raycast_oracle as R
import tsdf_raycast_scenes as RS
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


# ---- the oracle against a scalar transcription: one pixel, Python control flow, numpy float32 scalars (one rounding per operation)

def _scalar_sample(vol, dims, min_weight, a, b, z):
    """-> None (unobserved), or (t, corners[8], fr[3], (i0, j0, k0))"""
    g = [a[c] + z * b[c] for c in range(3)]
    f0 = [np.floor(x) for x in g]
    for c in range(3):
        if not (f0[c] >= F(0) and f0[c] <= F(dims[c] - 2)):
            return None
    i0, j0, k0 = (int(x) for x in f0)
    t = []
    for c in range(8):
        w = vol[k0 + (c >> 2), j0 + ((c >> 1) & 1), i0 + (c & 1)]
        if w[1] < min_weight:
            return None
        t.append(w[:1].view(F)[0])
    fr = [g[c] - f0[c] for c in range(3)]

    def lerp(lo, hi, f):
        d = hi - lo
        m = f * d
        return lo + m
    c00, c10, c01, c11 = lerp(t[0], t[1], fr[0]), lerp(t[2], t[3], fr[0]), lerp(t[4], t[5], fr[0]), lerp(t[6], t[7], fr[0])
    c0, c1 = lerp(c00, c10, fr[1]), lerp(c01, c11, fr[1])
    return lerp(c0, c1, fr[2]), t, fr, (i0, j0, k0), lerp


def scalar_pixel(vol, q, v, u, *, Ht, Wt, fx, fy, cx, cy, origin, voxel_size, min_weight=1, z_near=0.0, z_far, step):
    """-> (depth, (Gx, Gy, Gz), (r, g, b)) of one pixel"""
    Nz, Ny, Nx, _ = vol.shape
    dims = (Nx, Ny, Nz)
    q = [F(x) for x in q]
    vs = F(voxel_size)
    hole = (F(0), (F(0), F(0), F(0)), (0, 0, 0))
    with np.errstate(all="ignore"):
        dx, dy = (F(u) - F(cx)) / F(fx), (F(v) - F(cy)) / F(fy)
        a, b = [], []
        for c in range(3):
            w = (q[c] * dx + q[4 + c] * dy) + q[8 + c]
            o = -((q[c] * q[3] + q[4 + c] * q[7]) + q[8 + c] * q[11])
            a.append((o - F(origin[c])) / vs)
            b.append(w / vs)
        have_prev, t_prev, z_prev = False, F(0), F(0)
        for k in range(R.n_steps(z_near, z_far, step)):
            z_k = F(z_near) + F(k) * F(step)
            s = _scalar_sample(vol, dims, min_weight, a, b, z_k)
            if s is None:
                have_prev = False
                continue
            if have_prev and not (t_prev < 0) and s[0] < 0:
                break
            have_prev, t_prev, z_prev = True, s[0], z_k
        else:
            return hole
        z_hit = z_prev + (t_prev / (t_prev - s[0])) * (z_k - z_prev)
        s = _scalar_sample(vol, dims, min_weight, a, b, z_hit)
        if s is None:
            return hole
        _, t, fr, (i0, j0, k0), lerp = s
        G = (lerp(lerp(t[1] - t[0], t[3] - t[2], fr[1]), lerp(t[5] - t[4], t[7] - t[6], fr[1]), fr[2]),
             lerp(lerp(t[2] - t[0], t[3] - t[1], fr[0]), lerp(t[6] - t[4], t[7] - t[5], fr[0]), fr[2]),
             lerp(lerp(t[4] - t[0], t[5] - t[1], fr[0]), lerp(t[6] - t[2], t[7] - t[3], fr[0]), fr[1]))
    w = vol[k0 + int(fr[2] >= F(0.5)), j0 + int(fr[1] >= F(0.5)), i0 + int(fr[0] >= F(0.5))].view(np.uint32)
    rgb = tuple(int((int(c) + 128) >> 8) for c in (w[2] & 0xffff, w[2] >> 16, w[3] & 0xffff))
    return z_hit, G, rgb


def _bits(x):
    return np.asarray(x, F).view(np.int32).tolist()


def test_oracle_against_a_scalar_transcription_on_twenty_pixels():
    """a random volume with unobserved voxels under a rotated camera, and the ties scene: pixels chosen from the oracle's own diagnostics so
    that every kind is among them -- covered, never crossing, a crossing behind a reset, a crossing whose hit sample is unobserved -- and the
    image's corners"""
    g = RS.RANDOM_GRID
    vol = RS.random_volume(g["dims"], 5, unobserved=0.1)
    args = dict(**RS.CAM_ODD, **RS.place(g), **RS.march(g, step=0.03))
    r = R.raycast(vol, RS.POSES3[:2], **args)
    covered = r["depth"][:, 0] > 0
    kinds = [covered & ~r["reset"], covered & r["reset"], r["hit_unobserved"], r["steps"] < 0]
    pixels = [(0, 0, 0), (1, 0, 52), (0, 36, 0), (1, 36, 52)]
    for kind in kinds:
        found = np.argwhere(kind)
        assert len(found) >= 3
        pixels += [tuple(p) for p in found[:: max(1, len(found) // 3)][:3]]
    assert len(pixels) == 16
    for b, v, u in pixels:
        d, G, rgb = scalar_pixel(vol, RS.POSES3[b], v, u, **args)
        assert _bits(d) == _bits(r["depth"][b, 0, v, u]), (b, v, u)
        assert _bits(G) == _bits(r["gradients"][b, :, v, u]), (b, v, u)
        assert list(rgb) == r["image"][b, :, v, u].tolist(), (b, v, u)
    tv = RS.ties_volume()
    targs = dict(**RS.TIES_CAM, **RS.place(RS.TIES_GRID), z_near=0.0, z_far=2.25, step=0.125)
    rt = R.raycast(tv, RS.TIES_POSES, **targs)
    for b, v, u in ((0, 4, 4), (1, 4, 4), (2, 4, 4), (2, 3, 7)):
        d, G, rgb = scalar_pixel(tv, RS.TIES_POSES[b], v, u, **targs)
        assert _bits(d) == _bits(rt["depth"][b, 0, v, u]) and _bits(G) == _bits(rt["gradients"][b, :, v, u])
        assert list(rgb) == rt["image"][b, :, v, u].tolist()


def test_the_dyadic_plane_renders_exactly():
    """GRID_DYADIC, a plane at z = 2 seen from where it was fused: the tsdf is linear in z and constant in x and y, every number dyadic"""
    g = S.GRID_DYADIC
    vol, _ = O.integrate(O.empty(g["dims"]), *S.frames(["plane"], holes=False), np.array([S.IDENTITY], F), **RS.place(g), trunc=g["trunc"],
                         max_weight=64, **S.CAM)
    r = R.raycast(vol, np.array([S.IDENTITY], F), **RS.CAM_OWN, **RS.place(g), **RS.march(g))
    covered = r["depth"][0, 0] != 0
    assert r["count"][0] == covered.sum() and 0 < covered.sum() < covered.size
    assert (r["depth"][0, 0][covered] == F(2.0)).all()                        # within one voxel of 2.0 is what any ray caster owes; this is exact
    G = r["gradients"][0]
    assert (G[0][covered] == 0).all() and (G[1][covered] == 0).all() and (G[2][covered] < 0).all()
    assert (r["depth"][0, 0][~covered] == 0).all() and (G[:, ~covered] == 0).all() and (r["image"][0][:, ~covered] == 0).all()


def test_the_scenes_hold_what_the_gpu_tests_say_they_hold():
    tv = RS.ties_volume()
    place = RS.place(RS.TIES_GRID)
    r = R.raycast(tv, RS.TIES_POSES, **RS.TIES_CAM, **place, z_near=0.0, z_far=2.25, step=0.125)
    assert r["on_centre"][:, 4, 4].all() and r["on_edge"][0, 4, 4] and r["steps"][0, 4, 4] == -1
    assert r["t_prev"][1, 4, 4] == 0 and not np.signbit(r["t_prev"][1, 4, 4]) and r["depth"][1, 0, 4, 4] == F(1.25)
    assert r["t_prev"][2, 4, 4] == 0 and np.signbit(r["t_prev"][2, 4, 4]) and r["depth"][2, 0, 4, 4] == F(1.25)
    assert (r["fr_hit"][1, :, 4, 4] == 0).all()
    r = R.raycast(tv, RS.TIES_POSES, **RS.TIES_CAM, **place, z_near=0.0625, z_far=2.25, step=0.125)
    assert r["fr_hit"][2, 2, 4, 4] == F(0.5)
    away = R.raycast(RS.fuse(S.GRID_A), RS.POSES3, **RS.CAM_ODD, **RS.place(S.GRID_A), **RS.march(S.GRID_A))
    assert away["count"][2] == 0 and away["count"][0] > 0 and away["count"][1] > 0


# ---- the boundary

def _rdesc(**over):
    """a ray-cast descriptor that passes validation (the pointers are never dereferenced on the host)"""
    d = hip.TsdfRaycastDesc()
    d.volume, d.poses, d.depth, d.gradients, d.image, d.count = 1 << 20, 1 << 21, 1 << 22, 1 << 23, (1 << 24) + 1, 8192
    d.B, d.Ht, d.Wt, d.Nx, d.Ny, d.Nz, d.min_weight = 2, 37, 53, 19, 13, 11, 1
    d.fx, d.fy, d.cx, d.cy = 41.3, -39.7, 25.9, 17.3
    d.origin = (ctypes.c_double * 3)(-1.0, -1.0, 0.5)
    d.voxel_size = 0.05
    d.z_near, d.z_far, d.step = 0.0, 4.0, 0.1
    for k, v in over.items():
        if k.startswith("origin"):
            d.origin[int(k[6:])] = v
        else:
            setattr(d, k, v)
    return d


def test_symbols_version_and_header(lib):
    assert hasattr(lib, "s2m2_tsdf_raycast") and "s2m2_tsdf_raycast" in hip.SIGNATURES
    assert lib.s2m2_version() == 800 and hip.ABI_VERSION == 800
    header = open(os.path.join(ROOT, "include", "s2m2_hip.h")).read()
    assert int(re.search(r"#define S2M2_ABI_VERSION (\d+)", header).group(1)) == 800
    assert "s2m2_tsdf_raycast is NOT recorded" in header


def test_desc_has_the_layout_of_the_header(tmp_path):
    """every field: offset and size of the ctypes mirror against the struct compiled by gcc"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = [f[0] for f in hip.TsdfRaycastDesc._fields_]
    assert names == ["volume", "poses", "depth", "gradients", "image", "count", "B", "Ht", "Wt", "Nx", "Ny", "Nz", "min_weight", "fx", "fy", "cx",
                     "cy", "origin", "voxel_size", "z_near", "z_far", "step"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "s2m2_hip.h"', "int main(void) {", "  s2m2_tsdf_raycast_desc d;",
             '  printf("%zu\\n", sizeof(d));']
    lines += [f'  printf("{n} %zu %zu\\n", offsetof(s2m2_tsdf_raycast_desc, {n}), sizeof(d.{n}));' for n in names]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == ctypes.sizeof(hip.TsdfRaycastDesc)
    for n, line in zip(names, out[1:]):
        field, off, size = line.split()
        f = getattr(hip.TsdfRaycastDesc, n)
        assert (field, int(off), int(size)) == (n, f.offset, f.size)


RANGE = b"0 <= z_near < z_far and step > 0 are required"
RBAD = [
    (dict(volume=None), b"null pointer (volume)"),
    (dict(volume=(1 << 20) + 8), b"volume must be 16-byte aligned"),
    (dict(Ny=0), b"non-positive dims"),
    (dict(Nx=1024, Ny=1024, Nz=512), b"dims too large"),
    (dict(voxel_size=0.0), b"voxel_size must be finite and > 0"),
    (dict(voxel_size=1e-60), b"voxel_size must be finite and > 0"),
    (dict(origin2=INF), b"origin must be finite"),
    (dict(poses=None), b"null pointer (poses)"),
    (dict(poses=(1 << 21) + 2), b"poses must be 4-byte aligned"),
    (dict(depth=None, gradients=None, image=None, count=None), b"no output requested"),
    (dict(depth=(1 << 22) + 2), b"depth, gradients and count must be 4-byte aligned"),
    (dict(gradients=(1 << 23) + 1), b"depth, gradients and count must be 4-byte aligned"),
    (dict(count=8194), b"depth, gradients and count must be 4-byte aligned"),
    (dict(B=0), b"non-positive extents"),
    (dict(Ht=-1), b"non-positive extents"),
    (dict(Wt=0), b"non-positive extents"),
    (dict(B=1 << 16, Ht=1 << 8, Wt=1 << 7), b"extents too large"),
    (dict(B=1, Ht=1 << 16, Wt=1 << 15), b"extents too large"),
    (dict(B=1 << 30, Ht=1 << 30, Wt=1 << 30), b"extents too large"),
    (dict(fx=0.0), b"fx and fy must be finite and non-zero"),
    (dict(fy=1e-60), b"fx and fy must be finite and non-zero"),
    (dict(fx=NAN), b"fx and fy must be finite and non-zero"),
    (dict(fy=1e300), b"fx and fy must be finite and non-zero"),
    (dict(cx=INF), b"cx and cy must be finite"),
    (dict(cy=NAN), b"cx and cy must be finite"),
    (dict(min_weight=0), b"min_weight must be >= 1"),
    (dict(z_near=NAN), b"z_near, z_far and step must be finite"),
    (dict(z_far=INF), b"z_near, z_far and step must be finite"),
    (dict(step=1e300), b"z_near, z_far and step must be finite"),
    (dict(z_near=-0.5), RANGE),
    (dict(z_near=4.0), RANGE),
    (dict(z_near=4.0, z_far=4.0 + 1e-9), RANGE),                    # equal as fp32
    (dict(step=0.0), RANGE),
    (dict(step=-0.1), RANGE),
    (dict(step=1e-60), RANGE),                                       # zero as fp32
    (dict(z_far=65537.0, step=1.0), b"65537 steps from z_near to z_far (at most 65536)"),
    (dict(step=1e-30), b"steps from z_near to z_far (at most 65536)"),
]


@pytest.mark.parametrize("over,msg", RBAD, ids=[f"{'-'.join(o)}-{i}" for i, (o, _) in enumerate(RBAD)])
def test_validation_fails_before_any_device_call(lib, over, msg):
    assert lib.s2m2_tsdf_raycast(ctypes.byref(_rdesc(**over)), None) != 0
    assert msg in lib.s2m2_last_error(), lib.s2m2_last_error()
    assert lib.s2m2_last_error().startswith(b"tsdf_raycast: ")


def test_what_is_allowed(lib):
    """every output alone, a negative focal length, an unaligned image, z_near == 0, exactly 65536 steps, the largest extents: the first failure
    is the one put there on purpose"""
    alone = [dict({k: None for k in ("depth", "gradients", "image", "count") if k != keep}) for keep in ("depth", "gradients", "image", "count")]
    for over in alone + [dict(fx=-41.3), dict(z_far=65536.0, step=1.0), dict(z_near=1.0, z_far=1.0 + 65536 * 2.0 ** -10, step=2.0 ** -10),
                         dict(B=1, Ht=(1 << 31) - 1, Wt=1), dict(B=(1 << 31) - 1, Ht=1, Wt=1), dict(Nx=1, Ny=1, Nz=1)]:
        assert lib.s2m2_tsdf_raycast(ctypes.byref(_rdesc(min_weight=0, **over)), None) != 0
        assert b"tsdf_raycast: min_weight must be >= 1" in lib.s2m2_last_error(), (over, lib.s2m2_last_error())


def test_null_descriptor(lib):
    assert lib.s2m2_tsdf_raycast(None, None) != 0 and b"tsdf_raycast: null descriptor" in lib.s2m2_last_error()


def test_refused_while_a_plan_records(lib):
    plan = ctypes.c_void_p()
    assert lib.s2m2_plan_begin(ctypes.byref(plan)) == 0
    try:
        assert lib.s2m2_tsdf_raycast(ctypes.byref(_rdesc()), None) != 0
        assert b"not recorded in launch plans" in lib.s2m2_last_error()
        assert lib.s2m2_plan_launches(plan) == 0
    finally:
        lib.s2m2_plan_abort(plan)
        lib.s2m2_plan_destroy(plan)


# ---- the Python layers: every refusal comes before the library is reached

class _NoLibrary:
    """stands where the loaded library would: any entry point a wrapper reaches for fails the test"""

    def __getattr__(self, name):
        pytest.fail(f"the binding reached the library ({name}) with host operands")


def test_steps_is_the_entry_points_arithmetic():
    assert hip.tsdf_raycast_steps(0.0, 4.0, 0.1) == R.n_steps(0.0, 4.0, 0.1) == 40          # 0.1f is above 0.1: 39.99999940...
    assert hip.tsdf_raycast_steps(0.0, 65536.0, 1.0) == 65536 and hip.tsdf_raycast_steps(0.0, 65536.5, 1.0) == 65537
    assert hip.tsdf_raycast_steps(0.5, 0.75, 1.0) == 1
    for bad in ((-0.1, 1, 0.1), (1, 1, 0.1), (2, 1, 0.1), (0, 1, 0), (0, 1, -1), (NAN, 1, 0.1), (0, INF, 0.1), (0, 1, NAN), (0, 1e39, 0.1),
                (0, 1, 1e-60), (1.0, 1.0 + 1e-9, 0.1)):
        with pytest.raises(ValueError, match="z_near < z_far and step > 0"):
            hip.tsdf_raycast_steps(*bad)
    assert hip.tsdf_raycast_steps(0.0, 1.0, 1e-30) > hip.RAYCAST_MAX_STEPS == R.MAX_STEPS


def test_wrapper_refuses_bad_operands_before_the_library(monkeypatch):
    vol = torch.zeros(6, 5, 4, 4, dtype=torch.int32)
    poses = torch.zeros(2, 12)
    out = dict(depth=torch.zeros(2, 1, 7, 9), gradients=torch.zeros(2, 3, 7, 9), image=torch.zeros(2, 3, 7, 9, dtype=torch.uint8),
               count=torch.zeros(2, dtype=torch.int32))
    good = dict(Ht=7, Wt=9, fx=10.0, fy=10.0, cx=4.0, cy=3.0, origin=(0.0, 0.0, 1.0), voxel_size=0.1, z_far=2.0, step=0.05)
    with pytest.raises(ValueError, match="tsdf_raycast: operands must be device tensors"):
        hip.tsdf_raycast(vol, poses, **good, **out)
    monkeypatch.setattr(hip, "_lib", _NoLibrary())
    monkeypatch.setattr(hip, "_resident", lambda what, *ts: None)

    def refused(match, volume=vol, poses=poses, **over):
        kw = dict(good, **out)
        kw.update(over)
        with pytest.raises(ValueError, match=match):
            hip.tsdf_raycast(volume, poses, **kw)

    refused("volume must be a contiguous", volume=vol.float())
    refused("volume must be a contiguous", volume=torch.zeros(6, 5, 4, 3, dtype=torch.int32))
    refused("tensors must be contiguous", volume=torch.zeros(6, 5, 8, 4, dtype=torch.int32)[:, :, ::2])
    refused("poses must be a contiguous", poses=torch.zeros(2, 12, dtype=torch.float64))
    refused(r"poses must be a \(B, 12\)", poses=torch.zeros(2, 3, 4))
    refused("poses must be a contiguous", poses=torch.zeros(2, 13))
    refused(r"poses must be a \(B, 12\)", poses=torch.zeros(12))
    refused(r"poses must be a \(B, 12\)", poses=torch.zeros(0, 12))
    refused("depth must be a contiguous", depth=torch.zeros(2, 7, 9))
    refused("depth must be a contiguous", depth=torch.zeros(1, 1, 7, 9))
    refused("depth must be a contiguous", depth=torch.zeros(2, 1, 7, 9, dtype=torch.float16))
    refused("gradients must be a contiguous", gradients=torch.zeros(2, 1, 7, 9))
    refused("image must be a contiguous", image=torch.zeros(2, 3, 7, 9))
    refused("image must be a contiguous", image=torch.zeros(2, 3, 9, 7, dtype=torch.uint8))
    refused("count must be a contiguous", count=torch.zeros(3, dtype=torch.int32))
    refused("count must be a contiguous", count=torch.zeros(2, dtype=torch.int64))
    refused("no output requested", depth=None, gradients=None, image=None, count=None)
    refused("bad extents", Ht=0)
    refused("bad extents", Wt=7.5)
    refused("bad extents", Ht=1 << 20, Wt=1 << 10, depth=None, gradients=None, image=None)
    refused("fx must be finite and non-zero", fx=0.0)
    refused("fy must be finite and non-zero", fy=NAN)
    refused("fx must be finite and non-zero", fx=1e-60)
    refused("cx and cy must be finite", cy=INF)
    refused("origin is three finite numbers", origin=(0.0, NAN, 0.0))
    refused("voxel_size must be finite and > 0", voxel_size=0.0)
    refused("min_weight must be an integer >= 1", min_weight=0)
    refused("min_weight must be an integer >= 1", min_weight=1.5)
    refused("z_near < z_far and step > 0", z_near=-1.0)
    refused("z_near < z_far and step > 0", z_near=2.0)
    refused("z_near < z_far and step > 0", step=0.0)
    refused(r"65537 steps .*at most 65536", z_far=65537.0, step=1.0)


def test_volume_raycast_refuses_before_the_library(monkeypatch):
    monkeypatch.setattr(hip, "_lib", _NoLibrary())
    monkeypatch.setattr(hip, "_resident", lambda what, *ts: None)
    tv = cloud.TsdfVolume((4, 5, 6), 0.1, (0.0, 0.0, 1.0), device="cpu")
    cam = cloud.Camera(9, 7, 10.0, 10.0, 4.0, 3.0)
    assert tv.far_corner(np.eye(3), np.zeros(3)) == pytest.approx(math.sqrt(0.3 ** 2 + 0.4 ** 2 + 1.5 ** 2))
    assert tv.far_corner(np.eye(3)[None].repeat(2, 0), np.array([[0, 0, 0], [0, 0, 1.0]])) == pytest.approx(math.sqrt(0.3 ** 2 + 0.4 ** 2 + 2.5 ** 2))
    with pytest.raises(ValueError, match=r"TsdfVolume.raycast: R is \(3,3\) or \(1,3,3\)"):
        tv.raycast(cam, R=np.eye(4), t=np.zeros(3))
    with pytest.raises(ValueError, match=r"TsdfVolume.raycast: R is \(3,3\) or \(2,3,3\)"):
        tv.raycast(cam, R=np.eye(3)[None].repeat(2, 0), t=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="tsdf_raycast: 15[0-9]{4} steps .*at most 65536"):
        tv.raycast(cam, step=1e-5)                                  # the default z_far: the far corner, about 1.58
    with pytest.raises(ValueError, match="z_near < z_far and step > 0"):
        tv.raycast(cam, z_near=3.0)
    with pytest.raises(ValueError, match="min_weight must be an integer >= 1"):
        tv.raycast(cam, min_weight=0)
    r = cloud.TsdfRender(torch.zeros(2, 1, 3, 4), None, None, None, torch.eye(3)[None].repeat(2, 1, 1))
    with pytest.raises(ValueError, match="want_gradients=False"):
        r.normals()
    with pytest.raises(ValueError, match="want_count=False"):
        r.holes()
    G = torch.zeros(1, 3, 1, 2)
    G[0, :, 0, 1] = torch.tensor([0.0, 3.0, 4.0])
    turned = torch.tensor([[[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]])
    r = cloud.TsdfRender(torch.zeros(1, 1, 1, 2), G, None, torch.tensor([1], dtype=torch.int32), turned)
    assert r.holes() == 1 and r.normals()[0, :, 0, 0].tolist() == [0.0, 0.0, 0.0]
    assert torch.allclose(r.normals()[0, :, 0, 1], torch.tensor([0.6, 0.0, 0.8]))


# ---- the runner's option rules (usage errors, before the engine is loaded: no GPU needed)

POSE = "1,0,0,0,0,1,0,0,0,0,1,0"
TSDF = ["--tsdf-frames", "LIST", "--tsdf-dims", "19,13,11", "--tsdf-voxel", "0.1", "--tsdf-origin", "-0.9,-0.6,1.5", "--calib", CALIB,
        "--tsdf-ply", "t.ply"]
ENGINE = "cannot load the engine: engine_load: cannot open absent.s2m2"
NEED = "the --tsdf-render-* options need --tsdf-render"
POSE_MSG = "--tsdf-render: twelve finite numbers, [R | t] row-major, separated by commas"
RENDER_ROWS = [
    (TSDF + ["--tsdf-render", POSE, "--tsdf-render-depth", "d.f32"], ENGINE),
    (TSDF + ["--tsdf-render", POSE, "--tsdf-render-image", "i.u8"], ENGINE),
    (TSDF + ["--tsdf-mesh", "m.ply", "--tsdf-render", POSE, "--tsdf-render-depth", "d.f32", "--tsdf-render-image", "i.u8", "--tsdf-render-step", "0.05",
             "--tsdf-render-min-weight", "2"], ENGINE),
    (TSDF + ["--tsdf-render", POSE], "--tsdf-render needs --tsdf-render-depth or --tsdf-render-image"),
    (TSDF + ["--tsdf-render-depth", "d.f32"], NEED),
    (TSDF + ["--tsdf-render-image", "i.u8"], NEED),
    (TSDF + ["--tsdf-render-step", "0.05"], NEED),
    (TSDF + ["--tsdf-render-min-weight", "2"], NEED),
    (["--tsdf-render", POSE, "--tsdf-render-depth", "d.f32"], "the --tsdf-* options need --tsdf-frames"),
    ([a for a in TSDF if a not in ("--calib", CALIB)] + ["--tsdf-render", POSE, "--tsdf-render-depth", "d.f32"],
     "--tsdf-frames needs --tsdf-dims, --tsdf-voxel, --tsdf-origin, --calib and --tsdf-ply"),
    (TSDF + ["--tsdf-render", "1,0,0,0,0,1,0,0,0,0,1", "--tsdf-render-depth", "d.f32"], POSE_MSG),
    (TSDF + ["--tsdf-render", POSE + ",0", "--tsdf-render-depth", "d.f32"], POSE_MSG),
    (TSDF + ["--tsdf-render", "1,0,0,0,0,1,0,0,0,0,1,nan", "--tsdf-render-depth", "d.f32"], POSE_MSG),
    (TSDF + ["--tsdf-render", POSE.replace(",", " "), "--tsdf-render-depth", "d.f32"], POSE_MSG),
    (TSDF + ["--tsdf-render", POSE, "--tsdf-render-depth", "d.f32", "--tsdf-render-step", "0"], "--tsdf-render-step: a number > 0"),
    (TSDF + ["--tsdf-render", POSE, "--tsdf-render-depth", "d.f32", "--tsdf-render-step", "inf"], "--tsdf-render-step: a number > 0"),
    (TSDF + ["--tsdf-render", POSE, "--tsdf-render-depth", "d.f32", "--tsdf-render-min-weight", "0"], "--tsdf-render-min-weight: an integer in 1..32767"),
    (TSDF + ["--tsdf-render", POSE, "--tsdf-render-depth", "d.f32", "--tsdf-render-min-weight", "1.5"], "--tsdf-render-min-weight: an integer in 1..32767"),
    (TSDF + ["--tsdf-render"], "usage: s2m2_run_engine ENGINE LEFT RIGHT"),
]


@pytest.mark.parametrize("extra,msg", RENDER_ROWS, ids=[str(i) for i in range(len(RENDER_ROWS))])
def test_runner_tsdf_render_options(lib, tmp_path, extra, msg):
    """the mechanism of tests/test_runner_cpu.py: the runner itself, an engine file that does not exist as the last failure a complete command
    line can reach"""
    from s2m2_amd.build import RUNNER
    (tmp_path / "LIST").write_text("l0.f32 r0.f32 i0.u8 1 0 0 0 0 1 0 0 0 0 1 0\n")
    p = subprocess.run([RUNNER, "absent.s2m2"] + extra, capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 1 and msg in p.stderr, (extra, p.returncode, p.stderr)
    assert p.stderr.startswith("s2m2_run_engine: ") and p.stderr.count("\n") == 1


def test_the_usage_line_names_the_options():
    from s2m2_amd.build import RUNNER
    err = subprocess.run([RUNNER], capture_output=True, text=True, timeout=60).stderr
    for name in ("--tsdf-render POSE", "--tsdf-render-depth", "--tsdf-render-image", "--tsdf-render-step", "--tsdf-render-min-weight"):
        assert name in err
