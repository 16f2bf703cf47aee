"""CPU-side checks of K27 (include/s2m2_hip.h: s2m2_tsdf_track; s2m2_amd/cloud.py: TsdfVolume.track): the numpy oracle the GPU tests compare
against (against a plain scalar transcription of the per-pixel rule), what the scenes hold, and the boundary: symbols, descriptor layout, every
validation path of the entry point -- all of which return before any device call, there is no GPU here --, the wrappers' own errors, raised
before any library call, and the runner's option rules."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import tsdf_raycast_scenes as RS
import tsdf_scenes as S
import tsdf_track_oracle as T
import tsdf_track_scenes as TS
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


def _one(start, model=None, live="own", mpose=S.IDENTITY, cam="own", **over):
    """one iteration of the oracle on the tracking scene"""
    md, mg = model if model is not None else TS.render(cam=cam)[:2]
    (disp, occ, conf), kw = TS.live(live) if isinstance(live, str) else live
    kw = dict(kw, **TS.model_kw(cam), **dict(TS.GATES, **over))
    return T.iterate(disp, occ, conf, np.array(start, F), np.array(mpose, F), md, mg, **kw)


# ---- the oracle against a scalar transcription: one pixel, Python control flow, numpy float32 scalars (one rounding per operation)

def scalar_pixel(disp, occ, conf, q, m, md, mg, v, u, *, H, W, fx, fy, cx, cy, mfx, mfy, mcx, mcy, max_dist, baseline, doffs, depth_scale,
                 depth_trunc, conf_min, occ_min):
    """-> (class, J or None, r or None) of the live pixel (v, u)"""
    Hp, Wp = disp.shape
    oy, ox = (Hp - H) // 2, (Wp - W) // 2
    d, o, c = disp[oy + v, ox + u], occ[oy + v, ox + u], conf[oy + v, ox + u]
    q, m = [F(x) for x in q], [F(x) for x in m]
    Ht, Wt = md.shape
    with np.errstate(all="ignore"):
        if not (c > F(conf_min) and o > F(occ_min)):
            d = F(-1.0)
        depth = F(1e9) if d <= 0 else F(float(baseline) * float(fx)) / (d + F(doffs))
        z = depth / F(depth_scale)
        if not (z > 0 and z < F(depth_trunc)):
            return T.NOT_KEPT, None, None
        x = (F(u) - F(cx)) * z / F(fx)
        y = (F(v) - F(cy)) * z / F(fy)
        c0, c1, c2 = x - q[3], y - q[7], z - q[11]
        p = [(q[a] * c0 + q[4 + a] * c1) + q[8 + a] * c2 for a in range(3)]
        X = ((m[0] * p[0] + m[1] * p[1]) + m[2] * p[2]) + m[3]
        Y = ((m[4] * p[0] + m[5] * p[1]) + m[6] * p[2]) + m[7]
        Z = ((m[8] * p[0] + m[9] * p[1]) + m[10] * p[2]) + m[11]
        if not (Z > 0 and np.isfinite(Z)):
            return T.BEHIND, None, None
        fu = np.rint((F(mfx) * X) / Z + F(mcx))
        fv = np.rint((F(mfy) * Y) / Z + F(mcy))
        if not (fu >= 0 and fu < F(Wt) and fv >= 0 and fv < F(Ht)):
            return T.OUTSIDE, None, None
        dm = md[int(fv), int(fu)]
        if not dm > 0:
            return T.MODEL_HOLE, None, None
        g = [mg[a, int(fv), int(fu)] for a in range(3)]
        s = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        if not (s > 0 and np.isfinite(s)):
            return T.ZERO_GRADIENT, None, None
        ln = np.sqrt(s)
        n = [g[a] / ln for a in range(3)]
        mx = (fu - F(mcx)) * dm / F(mfx)
        my = (fv - F(mcy)) * dm / F(mfy)
        e = [mx - m[3], my - m[7], dm - m[11]]
        w = [(m[a] * e[0] + m[4 + a] * e[1]) + m[8 + a] * e[2] for a in range(3)]
        dd = [w[a] - p[a] for a in range(3)]
        if not ((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2] <= F(max_dist) * F(max_dist)):
            return T.FAR, None, None
        r = (n[0] * dd[0] + n[1] * dd[1]) + n[2] * dd[2]
        J = [p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]]
    return T.USED, J, r


def _bits(x):
    return np.asarray(x, F).view(np.int32).tolist()


def test_oracle_against_a_scalar_transcription_on_twenty_pixels():
    """three pixels of every class that the partial start through the odd model camera and the spoiled model produce, and the image's corners"""
    (disp, occ, conf), kw = TS.live()
    md, mg = TS.spoiled_model()
    cases = [(TS.PARTIAL, S.IDENTITY, md, mg, "own"), (TS.PARTIAL, S.IDENTITY, *TS.render(cam="odd")[:2], "odd"), (S.IDENTITY, RS.AWAY, md, mg, "own")]
    checked = 0
    for start, mpose, d, g, cam in cases:
        args = dict(kw, **TS.model_kw(cam), max_dist=TS.GATES["max_dist"])
        cls, J, r = T.rows(disp, occ, conf, np.array(start, F), np.array(mpose, F), d, g, **args)
        pixels = [(0, 0), (0, S.W - 1), (S.H - 1, 0), (S.H - 1, S.W - 1)]
        for k in range(7):
            found = np.flatnonzero(cls == k)
            pixels += [divmod(int(i), S.W) for i in found[:: max(1, len(found) // 3)][:3]]
        for v, u in pixels:
            k, Js, rs = scalar_pixel(disp, occ, conf, start, mpose, d, g, v, u, **args)
            assert k == cls[v * S.W + u], (cam, v, u)
            if k == T.USED:
                assert _bits(Js) == _bits(J[v * S.W + u]) and _bits(rs) == _bits(r[v * S.W + u]), (cam, v, u)
            checked += 1
    assert checked >= 20


def test_the_sums_are_the_exact_sums_rounded_once():
    from fractions import Fraction
    o = _one(S.IDENTITY)
    cls, J, r = T.rows(*TS.live()[0], np.array(S.IDENTITY, F), np.array(S.IDENTITY, F), *TS.render()[:2], **TS.live()[1], **TS.model_kw(),
                       max_dist=TS.GATES["max_dist"])
    used = cls == T.USED
    exact = sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(J[used, 0], J[used, 3]))
    assert o["sums"][3] == float(exact)                                    # A[0][3]
    assert o["row"][28] == used.sum() == o["count"] and (o["abs"] >= np.abs(o["sums"])).all()


# ---- what the scenes hold

def test_the_scenes_hold_what_the_gpu_tests_say_they_hold():
    seen = set()
    for start in (S.IDENTITY, TS.TRUE, TS.PARTIAL):
        o = _one(start)
        assert o["status"] == 0 and o["count"] >= 600 and o["kappa"] < 400 and o["bound"] < 2.0 ** -26
        seen |= set(np.unique(o["cls"]).tolist())
    assert 1400 <= _one(S.IDENTITY)["count"] <= 1600 and _one(S.IDENTITY)["kappa"] < 130
    seen |= set(np.unique(_one(S.IDENTITY, model=TS.spoiled_model())["cls"]).tolist())
    away = _one(S.IDENTITY, mpose=RS.AWAY)
    assert away["status"] == 1 and away["count"] == 0 and (away["cls"][away["cls"] != T.NOT_KEPT] == T.BEHIND).all()
    seen |= set(np.unique(away["cls"]).tolist())
    assert seen == set(range(7))                                           # every skip reason, and USED
    holes = _one(S.IDENTITY, model=(np.zeros((S.H, S.W), F), TS.render()[1]))
    assert holes["status"] == 1 and holes["count"] == 0
    assert _one(S.IDENTITY, max_trans=1e-6)["status"] == 3 and _one(TS.LOST)["status"] == 3
    assert _one(S.IDENTITY, max_rot=1e-6)["status"] == 3
    assert _one(S.IDENTITY, min_count=2000)["status"] == 1
    assert _one(S.IDENTITY, cam="odd")["status"] == 0
    # the dyadic plane seen from the identity: n = (0, 0, -1) exactly, so three columns of J are exactly zero and the third pivot is 0
    pd, pg = TS.plane_model()
    assert (pg[0] == 0).all() and (pg[1] == 0).all() and (pg[2][pd > 0] < 0).all()
    plane = _one(S.IDENTITY, model=(pd, pg), live=(TS.plane_live(), TS.live()[1]))
    assert plane["status"] == 2 and plane["count"] > 1000 and (plane["pose"] == np.array(S.IDENTITY, F)).all()
    A = T._sym(plane["sums"][:21])
    assert (A[2] == 0).all() and (A[3] == 0).all() and (A[4] == 0).all() and A[0, 0] > 0 and A[5, 5] == plane["count"]
    # four tiles of thirty rows with a partial last one, W % 4 != 0; a single row and a single column
    big, kwb = TS.live("big", 98, 140)
    assert kwb["H"] * kwb["W"] > 3 * 4096 and kwb["H"] % (4096 // kwb["W"]) != 0 and kwb["W"] % 4
    assert _one(S.IDENTITY, live=(big, kwb))["status"] == 0
    for cam, hp, wp in (("row", 7, 73), ("col", 51, 7)):
        o = _one(S.IDENTITY, live=TS.live(cam, hp, wp))
        assert o["count"] >= 6 and o["bound"] < 1e-6


def test_the_oracle_converges():
    (disp, occ, conf), kw = TS.live()
    md, mg, _ = TS.render()
    o = T.track(disp[None], occ[None], conf[None], np.array([S.IDENTITY], F), np.array([S.IDENTITY], F), md[None, None], mg[None], n_iters=8,
                **kw, **TS.model_kw(), **TS.GATES)
    r0, t0 = T.pose_errors(S.IDENTITY, TS.TRUE)
    r1, t1 = T.pose_errors(o["poses"][0], TS.TRUE)
    assert r1 <= r0 / 20 and t1 <= t0 / 10 and all(it["status"] == 0 for it in o["its"][0])
    assert _bits(o["residual"][0, 0]) == _bits(o["its"][0][-1]["residual"])
    R = o["poses"][0].reshape(3, 4)[:, :3].astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6


def test_update_moves_the_points_as_the_derivation_says():
    """p_w <- E p_w + v in the world: a point seen at p_cam under the new pose lies at E p + v of where it lay under the old one"""
    g = np.random.default_rng(3)
    pose = np.array(TS.PARTIAL, F)
    xi = g.uniform(-0.05, 0.05, 6)
    P = T.update(pose, xi).reshape(3, 4)
    old = pose.astype(np.float64).reshape(3, 4)
    pc = g.uniform(-1, 1, 3)
    w_old = old[:, :3].T @ (pc - old[:, 3])
    w_new = P[:, :3].T @ (pc - P[:, 3])
    assert np.abs(w_new - (T.rodrigues(xi[:3]) @ w_old + xi[3:])).max() < 1e-6      # (the re-orthonormalisation of a float32 R: 1e-7)
    assert np.abs(T.rodrigues(np.array([1e-5, 0, 0])) - T.rodrigues(np.array([1.0001e-4, 0, 0]))).max() < 1e-4


# ---- the boundary

def _tdesc(**over):
    """a tracking descriptor that passes validation (the pointers are never dereferenced on the host); keys with a `cloud_` prefix go to the
    embedded s2m2_cloud_desc"""
    d = hip.TsdfTrackDesc()
    c = d.cloud
    c.disp = c.occ = c.conf = 4096
    c.B, c.H, c.W, c.Hp, c.Wp, c.image_dtype = 2, 30, 50, 32, 64, 2
    c.fx, c.fy, c.cx, c.cy, c.baseline, c.doffs, c.depth_scale, c.depth_trunc, c.conf_min, c.occ_min = 1000.0, 1000.0, 25.0, 15.0, 100.0, 0.0, 1000.0, 3.0, 0.1, 0.5
    d.poses, d.model_poses, d.model_depth, d.model_gradients, d.systems, d.residual, d.workspace = 8192, 8448, 1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24
    d.Ht, d.Wt, d.min_count, d.n_iters = 37, 53, 6, 10
    d.mfx, d.mfy, d.mcx, d.mcy = 41.3, -39.7, 25.9, 17.3
    d.max_dist, d.max_rot, d.max_trans = 0.2, 0.3, 0.5
    for k, v in over.items():
        setattr(c if k.startswith("cloud_") else d, k[6:] if k.startswith("cloud_") else k, v)
    return d


def test_symbols_version_and_header(lib):
    for name in ("s2m2_tsdf_track", "s2m2_tsdf_track_workspace_bytes"):
        assert hasattr(lib, name) and name in hip.SIGNATURES
    assert lib.s2m2_version() == 800 and hip.ABI_VERSION == 800
    header = open(os.path.join(ROOT, "include", "s2m2_hip.h")).read()
    assert int(re.search(r"#define S2M2_ABI_VERSION (\d+)", header).group(1)) == 800
    assert "s2m2_tsdf_track is NOT recorded" in header


def test_workspace_bytes(lib):
    assert hip.tsdf_track_workspace_bytes(1, 45, 67) == 256                 # one tile of 32 doubles
    assert hip.tsdf_track_workspace_bytes(2, 92, 134) == 2 * 4 * 256 and hip.tsdf_track_workspace_bytes(1, 1024, 1216) == 342 * 256
    assert hip.tsdf_track_workspace_bytes(1, 21, 400) == 3 * 256            # tiles of ten rows
    assert hip.tsdf_track_workspace_bytes(3, 5, 5000) == 3 * 5 * 256        # a row wider than a tile: one row per tile
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (65536, 4, 4), (1, 1 << 16, 1 << 15)):
        with pytest.raises(ValueError, match="tsdf_track: bad extents"):
            hip.tsdf_track_workspace_bytes(*bad)


def test_desc_has_the_layout_of_the_header(tmp_path):
    """every field: offset and size of the ctypes mirror against the struct compiled by gcc"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = [f[0] for f in hip.TsdfTrackDesc._fields_]
    assert names == ["cloud", "poses", "model_poses", "model_depth", "model_gradients", "systems", "residual", "workspace", "Ht", "Wt", "min_count",
                     "n_iters", "mfx", "mfy", "mcx", "mcy", "max_dist", "max_rot", "max_trans"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "s2m2_hip.h"', "int main(void) {", "  s2m2_tsdf_track_desc d;",
             '  printf("%zu\\n", sizeof(d));']
    lines += [f'  printf("{n} %zu %zu\\n", offsetof(s2m2_tsdf_track_desc, {n}), sizeof(d.{n}));' for n in names]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == ctypes.sizeof(hip.TsdfTrackDesc)
    for n, line in zip(names, out[1:]):
        field, off, size = line.split()
        f = getattr(hip.TsdfTrackDesc, n)
        assert (field, int(off), int(size)) == (n, f.offset, f.size)


ALIGN4 = b"poses, model_poses, model_depth and model_gradients must be 4-byte aligned"
GATE = b"max_dist, max_rot and max_trans must be finite and > 0"
TBAD = [
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
    (dict(poses=None), b"null pointer (poses / model_poses)"),
    (dict(model_poses=None), b"null pointer (poses / model_poses)"),
    (dict(model_depth=None), b"null pointer (model_depth / model_gradients)"),
    (dict(model_gradients=None), b"null pointer (model_depth / model_gradients)"),
    (dict(poses=8194), ALIGN4),
    (dict(model_poses=8449), ALIGN4),
    (dict(model_depth=(1 << 20) + 2), ALIGN4),
    (dict(model_gradients=(1 << 21) + 3), ALIGN4),
    (dict(workspace=None), b"null workspace"),
    (dict(workspace=(1 << 24) + 4), b"workspace must be 8-byte aligned"),
    (dict(Ht=0), b"non-positive model extents"),
    (dict(Wt=-3), b"non-positive model extents"),
    (dict(Ht=1 << 16, Wt=1 << 15), b"model extents too large"),
    (dict(Ht=1 << 15, Wt=1 << 15), b"model extents too large"),             # B = 2
    (dict(mfx=0.0), b"mfx and mfy must be finite and non-zero"),
    (dict(mfy=1e-60), b"mfx and mfy must be finite and non-zero"),
    (dict(mfx=NAN), b"mfx and mfy must be finite and non-zero"),
    (dict(mfy=1e300), b"mfx and mfy must be finite and non-zero"),
    (dict(mcx=INF), b"mcx and mcy must be finite"),
    (dict(mcy=NAN), b"mcx and mcy must be finite"),
    (dict(max_dist=0.0), GATE),
    (dict(max_dist=NAN), GATE),
    (dict(max_dist=1e-60), GATE),
    (dict(max_rot=-0.1), GATE),
    (dict(max_rot=INF), GATE),
    (dict(max_trans=0.0), GATE),
    (dict(max_trans=1e300), GATE),
    (dict(min_count=5), b"min_count must be >= 6"),
    (dict(min_count=-1), b"min_count must be >= 6"),
    (dict(n_iters=0), b"n_iters must be 1..64"),
    (dict(n_iters=65), b"n_iters must be 1..64"),
    (dict(systems=(1 << 22) + 4), b"systems must be 8-byte aligned"),
    (dict(residual=(1 << 23) + 2), b"residual must be 4-byte aligned"),
]


@pytest.mark.parametrize("over,msg", TBAD, ids=[f"{'-'.join(o)}-{i}" for i, (o, _) in enumerate(TBAD)])
def test_validation_fails_before_any_device_call(lib, over, msg):
    assert lib.s2m2_tsdf_track(ctypes.byref(_tdesc(**over)), None) != 0
    assert msg in lib.s2m2_last_error(), lib.s2m2_last_error()
    assert lib.s2m2_last_error().startswith(b"tsdf_track: ")


def test_what_is_allowed(lib):
    """no image, no optional output, a negative model focal length, the extreme counts and extents: the first failure is the one put there on
    purpose"""
    for over in (dict(cloud_image=None), dict(systems=None), dict(mfx=-41.3), dict(n_iters=1), dict(n_iters=64), dict(min_count=6),
                 dict(cloud_B=1, Ht=(1 << 31) - 1, Wt=1), dict(cloud_depth=4098, cloud_count=4098, cloud_capacity=-1)):
        assert lib.s2m2_tsdf_track(ctypes.byref(_tdesc(residual=(1 << 23) + 2, **over)), None) != 0
        assert b"tsdf_track: residual must be 4-byte aligned" in lib.s2m2_last_error(), (over, lib.s2m2_last_error())


def test_null_descriptor(lib):
    assert lib.s2m2_tsdf_track(None, None) != 0 and b"tsdf_track: null descriptor" in lib.s2m2_last_error()


def test_refused_while_a_plan_records(lib):
    plan = ctypes.c_void_p()
    assert lib.s2m2_plan_begin(ctypes.byref(plan)) == 0
    try:
        assert lib.s2m2_tsdf_track(ctypes.byref(_tdesc()), None) != 0
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


def test_wrapper_refuses_bad_operands_before_the_library(lib, monkeypatch):
    maps = [torch.zeros(2, 1, 8, 12) for _ in range(3)]
    poses, mposes = torch.zeros(2, 12), torch.zeros(2, 12)
    md, mg = torch.zeros(2, 1, 7, 9), torch.zeros(2, 3, 7, 9)
    good = dict(H=6, W=11, fx=10.0, fy=10.0, cx=5.0, cy=3.0, baseline=1.0, mfx=10.0, mfy=10.0, mcx=4.0, mcy=3.0, max_dist=0.2, max_rot=0.2,
                max_trans=0.5, n_iters=3, workspace=torch.zeros(32, dtype=torch.float64), systems=torch.zeros(2, 3, 32, dtype=torch.float64),
                residual=torch.zeros(2, 1, 6, 11))
    with pytest.raises(ValueError, match="tsdf_track: operands must be device tensors"):
        hip.tsdf_track(*maps, poses, mposes, md, mg, **good)
    need = hip.tsdf_track_workspace_bytes(2, 6, 11)
    monkeypatch.setattr(hip, "_resident", lambda what, *ts: None)
    from s2m2_amd import hip_tsdf
    monkeypatch.setattr(hip_tsdf, "tsdf_track_workspace_bytes", lambda B, H, W: need)
    monkeypatch.setattr(hip, "_lib", _NoLibrary())

    def refused(match, disp=maps[0], poses=poses, mposes=mposes, md=md, mg=mg, **over):
        kw = dict(good)
        kw.update(over)
        with pytest.raises(ValueError, match=match):
            hip.tsdf_track(disp, maps[1], maps[2], poses, mposes, md, mg, **kw)

    refused(r"disp / occ / conf must be \(B,1,Hp,Wp\) fp32", disp=torch.zeros(2, 8, 12))
    refused("one shape", disp=torch.zeros(2, 1, 8, 16))
    refused("tensors must be contiguous", disp=torch.zeros(2, 1, 8, 24)[..., ::2])
    refused("the crop H=9 W=11 must be positive and no larger than the maps", H=9)
    refused("the crop H=6 W=0", W=0)
    refused("H and W must be integers", H=5.5)
    refused("tsdf_track: poses must be a contiguous", poses=torch.zeros(2, 13))
    refused("tsdf_track: poses must be a contiguous", poses=torch.zeros(2, 12, dtype=torch.float64))
    refused("tsdf_track: poses is required", poses=None)
    refused("model_poses must be a contiguous", mposes=torch.zeros(1, 12))
    refused(r"model_depth must be a \(B,1,Ht,Wt\)", md=torch.zeros(2, 7, 9))
    refused("model_depth must be a contiguous", md=torch.zeros(2, 2, 7, 9))
    refused("model_depth must be a contiguous", md=torch.zeros(2, 1, 7, 9, dtype=torch.float16))
    refused("model_gradients must be a contiguous", mg=torch.zeros(2, 3, 9, 7))
    refused("model_gradients is required", mg=None)
    refused("mfx must be finite and non-zero", mfx=0.0)
    refused("mfy must be finite and non-zero", mfy=NAN)
    refused("mcx and mcy must be finite", mcy=INF)
    refused("max_dist must be finite and > 0", max_dist=0.0)
    refused("max_rot must be finite and > 0", max_rot=NAN)
    refused("max_trans must be finite and > 0", max_trans=1e-60)
    refused("min_count must be an integer >= 6", min_count=5)
    refused("min_count must be an integer >= 6", min_count=6.5)
    refused(r"n_iters must be an integer in 1\.\.64", n_iters=0)
    refused(r"n_iters must be an integer in 1\.\.64", n_iters=65)
    refused("systems must be a contiguous", systems=torch.zeros(2, 2, 32, dtype=torch.float64))
    refused("systems must be a contiguous", systems=torch.zeros(2, 3, 32))
    refused("residual must be a contiguous", residual=torch.zeros(2, 1, 8, 12))
    refused(f"workspace of {need} bytes is required", workspace=torch.zeros(need // 8 - 1, dtype=torch.float64))
    refused(f"workspace of {need} bytes is required", workspace=None)


def test_volume_track_refuses_before_the_library(monkeypatch):
    monkeypatch.setattr(hip, "_lib", _NoLibrary())
    monkeypatch.setattr(hip, "_resident", lambda what, *ts: None)
    tv = cloud.TsdfVolume((4, 5, 6), 0.1, (0.0, 0.0, 1.0), device="cpu")
    maps = [torch.zeros(1, 1, 8, 12) for _ in range(3)]
    cam = cloud.Camera(9, 7, 10.0, 10.0, 4.0, 3.0)
    eye = torch.eye(3)[None]
    bare = cloud.TsdfRender(torch.zeros(1, 1, 7, 9), torch.zeros(1, 3, 7, 9), None, None, eye)          # the constructor of before: no poses
    assert bare.poses is None and bare.camera is None
    live = dict(fx=10.0, cx=5.0, cy=3.0, baseline=1.0)
    with pytest.raises(ValueError, match="the render must come from raycast"):
        tv.track(*maps, bare, R=np.eye(3), t=np.zeros(3), **live)
    full = cloud.TsdfRender(torch.zeros(1, 1, 7, 9), None, None, None, eye, torch.zeros(1, 12), cam)
    with pytest.raises(ValueError, match="the render must come from raycast"):
        tv.track(*maps, full, R=np.eye(3), t=np.zeros(3), **live)
    full = cloud.TsdfRender(torch.zeros(1, 1, 7, 9), torch.zeros(1, 3, 7, 9), None, None, eye, torch.zeros(1, 12), cam)
    with pytest.raises(ValueError, match="either as R and t or as poses"):
        tv.track(*maps, full, **live)
    with pytest.raises(ValueError, match="either as R and t or as poses"):
        tv.track(*maps, full, R=np.eye(3), t=np.zeros(3), poses=torch.zeros(1, 12), **live)
    with pytest.raises(ValueError, match=r"TsdfVolume.track: R is \(3,3\) or \(1,3,3\)"):
        tv.track(*maps, full, R=np.eye(4), t=np.zeros(3), **live)
    with pytest.raises(ValueError, match="either as R and t or as poses"):
        tv.integrate(*maps, torch.zeros(1, 3, 8, 12, dtype=torch.uint8), **live)
    tr = cloud.TsdfTrack(torch.arange(24, dtype=torch.float32).view(2, 12), None, None)
    assert tr.R[1].tolist() == [[12, 13, 14], [16, 17, 18], [20, 21, 22]] and tr.t[1].tolist() == [15, 19, 23]
    with pytest.raises(ValueError, match="want_systems=False"):
        tr.status()
    sysm = torch.zeros(1, 2, 32, dtype=torch.float64)
    sysm[0, 0, 28:30] = torch.tensor([7.0, 3.0], dtype=torch.float64)
    sysm[0, 1, 27:30] = torch.tensor([18.0, 8.0, 0.0], dtype=torch.float64)
    tr = cloud.TsdfTrack(torch.zeros(1, 12), sysm, None)
    assert tr.status() == 0 and tr.ok() and tr.count() == 8 and tr.rmse() == 1.5
    assert math.isnan(cloud.TsdfTrack(torch.zeros(1, 12), torch.zeros(1, 1, 32, dtype=torch.float64), None).rmse())


# ---- the runner's option rules (usage errors, before the engine is loaded: no GPU needed)

TSDF = ["--tsdf-frames", "LIST", "--tsdf-dims", "19,13,11", "--tsdf-voxel", "0.1", "--tsdf-origin", "-0.9,-0.6,1.5", "--calib", CALIB,
        "--tsdf-ply", "t.ply"]
ENGINE = "cannot load the engine: engine_load: cannot open absent.s2m2"
NEED = "--tsdf-track-iters, --tsdf-track-dist and --tsdf-poses-out need --tsdf-track"
LINE2 = "--tsdf-frames LIST: line 2: LEFT.f32 RIGHT.f32 IMAGE.u8 and twelve finite pose numbers"
TRACK_ROWS = [
    (TSDF + ["--tsdf-track"], ENGINE),
    (TSDF + ["--tsdf-track", "--tsdf-track-iters", "64", "--tsdf-track-dist", "0.3", "--tsdf-poses-out", "p.txt"], ENGINE),
    (TSDF + ["--tsdf-mesh", "m.ply", "--tsdf-track", "--tsdf-poses-out", "p.txt"], ENGINE),
    (TSDF, LINE2),                                                           # without --tsdf-track every line needs its pose
    (TSDF + ["--tsdf-track-iters", "5"], NEED),
    (TSDF + ["--tsdf-track-dist", "0.3"], NEED),
    (TSDF + ["--tsdf-poses-out", "p.txt"], NEED),
    (["--tsdf-track"], "the --tsdf-* options need --tsdf-frames"),
    (TSDF + ["--tsdf-track", "--tsdf-track-iters", "0"], "--tsdf-track-iters: an integer in 1..64"),
    (TSDF + ["--tsdf-track", "--tsdf-track-iters", "65"], "--tsdf-track-iters: an integer in 1..64"),
    (TSDF + ["--tsdf-track", "--tsdf-track-iters", "2.5"], "--tsdf-track-iters: an integer in 1..64"),
    (TSDF + ["--tsdf-track", "--tsdf-track-dist", "0"], "--tsdf-track-dist: a number > 0"),
    (TSDF + ["--tsdf-track", "--tsdf-track-dist", "nan"], "--tsdf-track-dist: a number > 0"),
    (TSDF + ["--tsdf-track", "--tsdf-track-iters"], "usage: s2m2_run_engine ENGINE LEFT RIGHT"),
]


@pytest.mark.parametrize("extra,msg", TRACK_ROWS, ids=[str(i) for i in range(len(TRACK_ROWS))])
def test_runner_tsdf_track_options(lib, tmp_path, extra, msg):
    """the mechanism of tests/test_runner_cpu.py: the runner itself, an engine file that does not exist as the last failure a complete command
    line can reach.  The second line of LIST has no pose and the third has one: both are fine with --tsdf-track, and only then"""
    from s2m2_amd.build import RUNNER
    (tmp_path / "LIST").write_text("l0.f32 r0.f32 i0.u8 1 0 0 0 0 1 0 0 0 0 1 0\nl1.f32 r1.f32 i1.u8\nl2.f32 r2.f32 i2.u8 1 0 0 0 0 1 0 0 0 0 1 0\n")
    p = subprocess.run([RUNNER, "absent.s2m2"] + extra, capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 1 and msg in p.stderr, (extra, p.returncode, p.stderr)
    assert p.stderr.startswith("s2m2_run_engine: ") and p.stderr.count("\n") == 1


def test_runner_refuses_a_first_line_without_a_pose_and_a_partial_pose(lib, tmp_path):
    from s2m2_amd.build import RUNNER
    for text, line in (("l0.f32 r0.f32 i0.u8\n", 1), ("l0.f32 r0.f32 i0.u8 1 0 0 0 0 1 0 0 0 0 1 0\nl1.f32 r1.f32 i1.u8 1 0 0\n", 2)):
        (tmp_path / "LIST").write_text(text)
        p = subprocess.run([RUNNER, "absent.s2m2"] + TSDF + ["--tsdf-track"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert p.returncode == 1 and f"--tsdf-frames LIST: line {line}: LEFT.f32 RIGHT.f32 IMAGE.u8 and twelve finite pose numbers" in p.stderr


def test_the_usage_line_names_the_options():
    from s2m2_amd.build import RUNNER
    err = subprocess.run([RUNNER], capture_output=True, text=True, timeout=60).stderr
    for name in ("--tsdf-track ", "--tsdf-track-iters N", "--tsdf-track-dist D", "--tsdf-poses-out FILE"):
        assert name in err
