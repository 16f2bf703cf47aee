"""K27 on the GPU (include/s2m2_hip.h: s2m2_tsdf_track; s2m2_amd/cloud.py: TsdfVolume.track) against the numpy oracle of
tests/tsdf_track_oracle.py -- never against the code under test.

What one iteration owes: the count, the status and the residual map as BYTES (the per-pixel rule is fp32 with one rounding per operation); each
of the 28 sums within gamma_{n-1} * sum |term| of the exact sum, which holds for ANY order of n - 1 additions in double (n = count, gamma_k =
k u / (1 - k u), u = 2^-53); each entry of the new pose within one fp32 spacing of the oracle's unrounded float64 pose plus the oracle's bound
of what such a change of the sums can do to it (tsdf_track_oracle.pose_bound).  Several iterations are pinned by chaining: n_iters = 8 is eight
calls of n_iters = 1, byte for byte.

Every scene asserts FROM THE ORACLE that it holds what it is meant to hold before anything is compared.  The pose buffer, both outputs and the
workspace are poisoned before each call, each output with a guard behind it; the guards, and the outputs that a call does not request, must
still hold the poison."""
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import tsdf_oracle as O
import tsdf_raycast_oracle as R
import tsdf_raycast_scenes as RS
import tsdf_scenes as S
import tsdf_track_oracle as T
import tsdf_track_scenes as TS
from s2m2_amd import cloud, utils

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64
POISON = dict(systems=-7.25e77, residual=0x7fc00123)
ALL = ("systems", "residual")


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _stack(*pairs):
    """pairs of (maps, kw) with one shape -> disp, occ, conf (B,Hp,Wp) and the common kw"""
    maps, kws = zip(*pairs)
    assert all(k == kws[0] for k in kws)
    return [np.stack([m[i] for m in maps]) for i in range(3)], kws[0]


def _gpu(hip, maps, poses, mposes, md, mg, which=ALL, *, n_iters=1, **kw):
    """one call: maps (B,Hp,Wp) x 3, poses / mposes (B,12), md (B,1,Ht,Wt), mg (B,3,Ht,Wt) -> poses (B,12), systems, residual (None where
    not requested) as numpy; the guards and the outputs not requested are checked for their poison here"""
    B, H, W = len(poses), kw["H"], kw["W"]
    n = dict(systems=B * n_iters * 32, residual=B * H * W)
    flat = dict(systems=torch.full((n["systems"] + GUARD,), POISON["systems"], dtype=torch.float64, device="cuda"),
                residual=torch.full((n["residual"] + GUARD,), POISON["residual"], dtype=torch.int32, device="cuda"))
    view = dict(systems=flat["systems"][:n["systems"]].view(B, n_iters, 32), residual=flat["residual"][:n["residual"]].view(B, 1, H, W).view(torch.float32))
    pflat = torch.full((B * 12 + GUARD,), -3.5e33, device="cuda")
    pbuf = pflat[:B * 12].view(B, 12)
    pbuf.copy_(_dev(np.asarray(poses, F)))
    ws = torch.full((hip.tsdf_track_workspace_bytes(B, H, W) // 8 + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    hip.tsdf_track(*[_dev(m[:, None]) for m in maps], pbuf, _dev(np.asarray(mposes, F)), _dev(md), _dev(mg), n_iters=n_iters, workspace=ws[:-GUARD],
                   **kw, **{k: view[k] for k in which})
    torch.cuda.synchronize()
    assert (pflat[B * 12:] == -3.5e33).all(), "written behind poses"
    assert torch.isnan(ws[-GUARD:]).all(), "written behind the workspace"
    for key in ALL:
        tail = flat[key][n[key]:]
        assert (tail == POISON[key]).all(), f"written behind {key}"
        if key not in which:
            assert (flat[key] == POISON[key]).all(), f"{key} was not requested"
    return pbuf.cpu().numpy(), *(view[k].cpu().numpy() if k in which else None for k in ALL)


def _bytes(a):
    return np.ascontiguousarray(a).tobytes()


def _check1(hip, maps, poses, mposes, md, mg, *, condition=None, **kw):
    """one iteration against the oracle -> the oracle's dicts, one per pair"""
    poses, mposes = np.asarray(poses, F), np.asarray(mposes, F)
    got_p, got_s, got_r = _gpu(hip, maps, poses, mposes, md, mg, n_iters=1, **kw)
    outs = []
    for b in range(len(poses)):
        o = T.iterate(maps[0][b], maps[1][b], maps[2][b], poses[b], mposes[b], md[b, 0], mg[b], **kw)
        row = got_s[b, 0]
        print(f"[tsdf track] pair {b}: count {o['count']} (gpu {row[28]:.0f}) status {o['status']} (gpu {row[29]:.0f}) kappa {o['kappa']:.3g} "
              f"bound {o['bound']:.3g}")
        assert _bytes(row[28:30]) == _bytes(o["row"][28:30]), "count / status"
        assert _bytes(got_r[b, 0].view(np.int32)) == _bytes(o["residual"].view(np.int32)), "residual"
        n = o["count"]
        if n:
            err, lim = T.sum_errors(o["J"], o["r"], row[:28]), T.gamma(max(n - 1, 1)) * o["abs"]
            print(f"[tsdf track]   sums: largest error / bound {np.max(err / np.maximum(lim, 1e-300)):.3g}")
            assert (err <= lim).all(), (err, lim)
        else:
            assert not row[:28].any()
        if o["status"] == 0:
            if condition is not None:
                assert o["bound"] < condition                                  # the condition, from the oracle
            tol = np.spacing(np.abs(o["P"]).astype(F)).astype(np.float64) + o["bound"]
            d = np.abs(got_p[b].astype(np.float64) - o["P"])
            print(f"[tsdf track]   pose: largest error / tolerance {np.max(d / tol):.3g}")
            assert (d <= tol).all(), (got_p[b], o["P"])
            assert abs(row[30] - o["wn"]) <= 1e-9 and abs(row[31] - o["vn"]) <= 1e-9
        else:
            assert _bytes(got_p[b]) == _bytes(poses[b]), "the pose of a refused step changed"
            if o["status"] in (1, 2):
                assert row[30] == 0 and row[31] == 0
        outs.append(o)
    return outs


def _scene(live="own", cam="own", pad=(51, 73)):
    (disp, occ, conf), kw = TS.live(live, *pad)
    md, mg, _ = TS.render(cam=cam)
    return [disp[None], occ[None], conf[None]], md[None, None], mg[None], dict(kw, **TS.model_kw(cam), **TS.GATES)


IDENT = np.array([S.IDENTITY], F)


# ---- 1. one iteration

@pytest.mark.parametrize("start", ["IDENTITY", "TRUE", "PARTIAL"])
def test_one_iteration(hip, start):
    """from the prototype's offset (the model's own pose), from the true pose, and from a pose with partial overlap"""
    maps, md, mg, kw = _scene()
    pose = np.array([S.IDENTITY if start == "IDENTITY" else getattr(TS, start)], F)
    o, = _check1(hip, maps, pose, IDENT, md, mg, condition=2.0 ** -26, **kw)
    assert o["status"] == 0 and o["count"] >= 600
    if start == "PARTIAL":
        assert (o["cls"] == T.OUTSIDE).sum() > 100 and (o["cls"] == T.FAR).sum() > 100


def test_a_spoiled_model_and_a_model_camera_of_its_own(hip):
    """zero, NaN and Inf gradients, NaN, negative and Inf depths never become a correspondence; CAM_ODD differs from the live camera"""
    maps, _, _, kw = _scene()
    md, mg = TS.spoiled_model()
    o, = _check1(hip, maps, IDENT, IDENT, md[None, None], mg[None], **kw)
    assert o["status"] == 0 and (o["cls"] == T.ZERO_GRADIENT).sum() > 20 and (o["cls"] == T.FAR).sum() > 0
    maps, md, mg, kw = _scene(cam="odd")
    o, = _check1(hip, maps, IDENT, IDENT, md, mg, condition=2.0 ** -26, **kw)
    assert o["status"] == 0 and md.shape[-2:] == (37, 53)


# ---- 2. chaining, reproducibility, convergence

def test_eight_iterations_are_eight_calls(hip):
    maps, md, mg, kw = _scene()
    p8, s8, r8 = _gpu(hip, maps, IDENT, IDENT, md, mg, n_iters=8, **kw)
    p, rows = IDENT, []
    for _ in range(8):
        p, s, r = _gpu(hip, maps, p, IDENT, md, mg, n_iters=1, **kw)
        rows.append(s[:, 0])
    assert _bytes(p8) == _bytes(p) and _bytes(s8) == _bytes(np.stack(rows, 1)) and _bytes(r8.view(np.int32)) == _bytes(r.view(np.int32))
    assert (s8[0, :, 29] == 0).all() and _bytes(p8) != _bytes(IDENT)


def test_convergence(hip):
    """a condition, not a measurement: from the prototype's offset both errors fall to a fifth at the most (the oracle reaches 1/25 and 1/14)"""
    maps, md, mg, kw = _scene()
    r0, t0 = T.pose_errors(S.IDENTITY, TS.TRUE)
    o = T.track(*maps, IDENT, IDENT, md, mg, n_iters=8, **kw)
    ro, to = T.pose_errors(o["poses"][0], TS.TRUE)
    assert ro <= r0 / 5 and to <= t0 / 5                                       # of the oracle first
    p, s, _ = _gpu(hip, maps, IDENT, IDENT, md, mg, n_iters=8, **kw)
    r1, t1 = T.pose_errors(p[0], TS.TRUE)
    print(f"[tsdf track] rotation {r0:.3g} -> {r1:.3g} (oracle {ro:.3g}), translation {t0:.3g} -> {t1:.3g} (oracle {to:.3g})")
    assert r1 <= r0 / 5 and t1 <= t0 / 5 and (s[0, :, 29] == 0).all()


def test_two_runs_and_a_graph_replay(hip):
    maps, md, mg, kw = _scene("big", pad=(98, 140))
    ref = _gpu(hip, maps, IDENT, IDENT, md, mg, n_iters=4, **kw)
    again = _gpu(hip, maps, IDENT, IDENT, md, mg, n_iters=4, **kw)
    assert all(_bytes(a) == _bytes(b) for a, b in zip(ref, again)) and (ref[1][0, :, 29] == 0).all()
    dev = [_dev(m[:, None]) for m in maps]
    pbuf, mp, dmd, dmg = _dev(IDENT), _dev(IDENT), _dev(md), _dev(mg)
    systems = torch.zeros((1, 4, 32), dtype=torch.float64, device="cuda")
    residual = torch.zeros((1, 1, kw["H"], kw["W"]), device="cuda")
    ws = torch.empty((hip.tsdf_track_workspace_bytes(1, kw["H"], kw["W"]) // 8,), dtype=torch.float64, device="cuda")

    def run():
        hip.tsdf_track(*dev, pbuf, mp, dmd, dmg, n_iters=4, workspace=ws, systems=systems, residual=residual, **kw)

    run()                                                                      # the warm-up of the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()                                             # (one stream, no side branches)
    with torch.cuda.graph(graph):
        run()
    for _ in range(2):
        pbuf.copy_(_dev(IDENT))
        systems.fill_(-1.0)
        residual.fill_(-1.0)
        ws.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = (pbuf.cpu().numpy(), systems.cpu().numpy(), residual.cpu().numpy())
        assert all(_bytes(a) == _bytes(b) for a, b in zip(ref, got))


# ---- 3. degenerate input, exactly

def _plane():
    pd, pg = TS.plane_model()
    disp, occ, conf = TS.plane_live()
    return ([disp[None], occ[None], conf[None]], TS.live()[1]), pd[None, None], pg[None]


def test_the_dyadic_plane_is_singular(hip):
    """gradients (0, 0, g) exactly: three columns of J are exactly zero, the third pivot is exactly 0 -> status 2, the pose byte-unchanged"""
    (maps, lkw), pd, pg = _plane()
    kw = dict(lkw, **TS.model_kw(), **TS.GATES)
    o, = _check1(hip, maps, IDENT, IDENT, pd, pg, **kw)
    assert o["status"] == 2 and o["count"] > 1000
    p, s, _ = _gpu(hip, maps, IDENT, IDENT, pd, pg, n_iters=3, **kw)
    assert _bytes(p) == _bytes(IDENT) and (s[0, :, 29] == 2).all() and _bytes(s[0, 0]) == _bytes(s[0, 2])
    A = T._sym(s[0, 0, :21])
    assert not A[2].any() and not A[3].any() and not A[4].any()


def test_too_few_and_too_long(hip):
    maps, md, mg, kw = _scene()
    o, = _check1(hip, maps, IDENT, IDENT, np.zeros_like(md), mg, **kw)         # an all-hole model
    assert o["status"] == 1 and o["count"] == 0
    o, = _check1(hip, maps, IDENT, np.array([RS.AWAY], F), md, mg, **kw)       # every live point behind the model camera
    assert o["status"] == 1 and o["count"] == 0
    o, = _check1(hip, maps, IDENT, IDENT, md, mg, **dict(kw, min_count=2000))
    assert o["status"] == 1 and o["count"] > 1400
    o, = _check1(hip, maps, IDENT, IDENT, md, mg, **dict(kw, max_trans=1e-6))
    assert o["status"] == 3 and o["vn"] > 1e-6
    o, = _check1(hip, maps, IDENT, IDENT, md, mg, **dict(kw, max_rot=1e-6))
    assert o["status"] == 3
    o, = _check1(hip, maps, np.array([TS.LOST], F), IDENT, md, mg, **kw)
    assert o["status"] == 3


@pytest.mark.parametrize("what", ["pose", "model_pose", "disp", "depth", "gradients"])
def test_non_finite_input_forms_no_address(hip, what):
    """NaN / Inf poses and maps end in status 1 or 2 (here: no correspondence is left, status 1), the pose is unchanged and the guards hold"""
    maps, md, mg, kw = _scene()
    maps = [m.copy() for m in maps]
    pose, mpose, md, mg = IDENT.copy(), IDENT.copy(), md.copy(), mg.copy()
    vals = np.array((np.nan, np.inf, -np.inf), F)
    if what == "pose":
        pose[0, [1, 7, 10]] = vals
    elif what == "model_pose":
        mpose[0, [0, 6, 11]] = vals
    elif what == "disp":
        maps[0][0] = vals[np.arange(maps[0][0].size) % 3].reshape(maps[0][0].shape)
    elif what == "depth":
        md[:] = vals[np.arange(md.size) % 3].reshape(md.shape)
    else:
        mg[:] = vals[np.arange(mg.size) % 3].reshape(mg.shape)
    o, = _check1(hip, maps, pose, mpose, md, mg, **kw)
    assert o["status"] in (1, 2) and o["count"] == 0


def test_two_pairs_are_independent(hip):
    """the tracking scene and the singular plane in one call: each pair as if it were alone"""
    track, plane = (TS.live()), (TS.plane_live(), TS.live()[1])
    maps, lkw = _stack(track, plane)
    pd, pg = TS.plane_model()
    md, mg, _ = TS.render()
    kw = dict(lkw, **TS.model_kw(), **TS.GATES)
    poses = np.array([S.IDENTITY, S.IDENTITY], F)
    outs = _check1(hip, maps, poses, poses, np.stack([md, pd])[:, None], np.stack([mg, pg]), **kw)
    assert [o["status"] for o in outs] == [0, 2]
    p2, s2, r2 = _gpu(hip, maps, poses, poses, np.stack([md, pd])[:, None], np.stack([mg, pg]), n_iters=3, **kw)
    p1, s1, r1 = _gpu(hip, [m[:1] for m in maps], IDENT, IDENT, md[None, None], mg[None], n_iters=3, **kw)
    assert _bytes(p2[0]) == _bytes(p1[0]) and _bytes(s2[0]) == _bytes(s1[0]) and _bytes(r2[0].view(np.int32)) == _bytes(r1[0].view(np.int32))
    assert _bytes(p2[1]) == _bytes(poses[1]) and (s2[1, :, 29] == 2).all()


# ---- 4. tiling

@pytest.mark.parametrize("live,pad", [("big", (98, 140)), ("big", (92, 134)), ("row", (7, 73)), ("col", (51, 7)), ("own", (45, 68))])
def test_tiling(hip, live, pad):
    """92 x 134: four tiles of thirty rows, the last of two, W % 4 == 2 -- with a padded map of a multiple of four columns and an odd crop offset
    (one 16-byte load per thread) and unpadded (per pixel); one row; one column; no padding above and one column to the right.  The padded
    border holds kept pixels that must not be read"""
    maps, md, mg, kw = _scene(live, pad=pad)
    o, = _check1(hip, maps, IDENT, IDENT, md, mg, **kw)
    assert o["count"] >= 6 and o["bound"] < 1e-6
    if live == "big":
        assert hip.tsdf_track_workspace_bytes(1, kw["H"], kw["W"]) == 4 * 256 and o["status"] == 0


# ---- 5. every subset of the outputs

@pytest.mark.parametrize("which", [c for n in range(0, 3) for c in itertools.combinations(ALL, n)], ids=lambda w: "-".join(w) or "none")
def test_every_subset_of_the_outputs(hip, which):
    maps, md, mg, kw = _scene()
    ref = _gpu(hip, maps, IDENT, IDENT, md, mg, n_iters=2, **kw)
    got = _gpu(hip, maps, IDENT, IDENT, md, mg, which, n_iters=2, **kw)
    assert _bytes(got[0]) == _bytes(ref[0])
    for key, g, e in zip(ALL, got[1:], ref[1:]):
        assert (g is None) == (key not in which) and (g is None or _bytes(g) == _bytes(e))


# ---- 6. the Python layer

def _volume(vol=None):
    tv = cloud.TsdfVolume(TS.GRID["dims"], TS.GRID["voxel_size"], TS.GRID["origin"], trunc=TS.GRID["trunc"])
    tv.buffer.copy_(_dev(TS.volume() if vol is None else vol))
    return tv


CAMERA = dict(fx=S.CAM["fx"], cx=S.CAM["cx"], cy=S.CAM["cy"], baseline=S.CAM["baseline"], depth_scale=S.CAM["depth_scale"], depth_trunc=S.CAM["depth_trunc"])


def test_tsdf_volume_track_end_to_end(hip):
    maps, md, mg, kw = _scene()
    tv = _volume()
    cam = cloud.Camera(S.W, S.H, S.CAM["fx"], S.CAM["fy"], S.CAM["cx"], S.CAM["cy"])
    render = tv.raycast(cam, np.eye(3), np.zeros(3), z_far=4.0)
    assert render.camera is cam and tuple(render.poses.shape) == (1, 12)
    assert _bytes(render.depth.cpu().numpy()) == _bytes(md) and _bytes(render.gradients_buf.cpu().numpy()) == _bytes(mg)
    dev = [_dev(m[:, None]) for m in maps]
    tr = tv.track(*dev, render, R=np.eye(3), t=np.zeros(3), H=S.H, W=S.W, **CAMERA, n_iters=8, min_count=6, max_rot=0.5, max_trans=0.5,
                  want_residual=True)
    e = _gpu(hip, maps, IDENT, IDENT, md, mg, n_iters=8, **kw)                 # max_dist: the default is trunc
    assert _bytes(tr.poses.cpu().numpy()) == _bytes(e[0]) and _bytes(tr.systems.cpu().numpy()) == _bytes(e[1])
    assert _bytes(tr.residual.cpu().numpy().view(np.int32)) == _bytes(e[2].view(np.int32))
    assert tr.ok() and tr.status() == 0 and tr.count() == int(e[1][0, -1, 28]) and tr.rmse() == pytest.approx(np.sqrt(e[1][0, -1, 27] / e[1][0, -1, 28]))
    assert torch.equal(tr.R[0], tr.poses.view(3, 4)[:, :3]) and torch.equal(tr.t[0], tr.poses.view(3, 4)[:, 3])
    # a device buffer refined in place, the defaults of the gates, no outputs; the tracked pose feeds integrate without a copy
    buf = _dev(IDENT)
    tr2 = tv.track(*dev, render, poses=buf, H=S.H, W=S.W, **CAMERA, n_iters=8, want_systems=False)
    assert tr2.poses is buf and tr2.systems is None and tr2.residual is None
    d = _gpu(hip, maps, IDENT, IDENT, md, mg, n_iters=8, **dict(kw, min_count=100, max_rot=0.2, max_trans=4 * TS.GRID["trunc"]))
    assert _bytes(buf.cpu().numpy()) == _bytes(d[0])
    with pytest.raises(ValueError, match="want_systems=False"):
        tr2.ok()
    img = torch.zeros((1, 3, S.H, S.W), dtype=torch.uint8, device="cuda")
    tv.integrate(*dev, img, poses=buf, **CAMERA, carve=True)
    want, _ = O.integrate(TS.volume(), *maps, np.zeros((1, 3, S.H, S.W), np.uint8), d[0], **RS.place(TS.GRID), trunc=TS.GRID["trunc"], max_weight=64,
                          carve=True, **S.CAM)
    assert _bytes(tv.buffer.cpu().numpy()) == _bytes(want)


def test_utils_track_tsdf(hip):
    """integrate_tsdf's conventions: halved intrinsics, fx for both focal lengths, the disparity as all three maps"""
    tv = _volume()
    calib = dict(cam0=np.array([[128.0, 0, 67.0], [0, 120.0, 45.0], [0, 0, 1]]), baseline=15.625, doffs=0.0, width=2 * S.W, height=2 * S.H)
    (disp, occ, conf), kw = TS.live(Hp=S.H, Wp=S.W)
    Rm, t, ok = utils.track_tsdf(tv, disp, calib, np.eye(3), np.zeros(3), depth_trunc=10.0, n_iters=8, min_count=6, max_rot=0.5, max_trans=0.5)
    # z = baseline * fx / d / 1000 with baseline * fx = 15.625 * 64 = 1000: the scene's z = 1 / d
    far = R.raycast(TS.volume(), IDENT, **RS.CAM_OWN, **RS.place(TS.GRID), z_near=0.0, z_far=tv.far_corner(np.eye(3), np.zeros(3)), step=TS.GRID["trunc"] / 2)
    args = dict(kw, baseline=15.625, depth_scale=1000.0, **TS.model_kw(), **TS.GATES)
    e = T.track(disp[None], disp[None], disp[None], IDENT, IDENT, far["depth"], far["gradients"], n_iters=8, filtered=False, **args)
    assert ok and all(it["status"] == 0 for it in e["its"][0]) and e["its"][0][-1]["count"] > 1400
    got = np.concatenate([Rm.cpu().numpy(), t.cpu().numpy()[:, None]], 1).ravel()
    assert np.abs(got - e["poses"][0]).max() < 1e-4                            # (eight chained iterations: loose; a plumbing test)
    r0, t0 = T.pose_errors(S.IDENTITY, TS.TRUE)
    r1, t1 = T.pose_errors(got, TS.TRUE)
    assert r1 <= r0 / 5 and t1 <= t0 / 5


# ---- 7. the closed loop

def test_raycast_track_integrate_captured_once(hip):
    """three frames of a moving camera: raycast from the last pose, track, integrate with the tracked pose -- captured once and replayed, with
    only the maps rewritten; no pose leaves the device.  The volume after every frame is the oracle's integrate of the frame at the pose the
    device tracked (bytes); the last pose satisfies the convergence condition, asserted of the oracle chain first"""
    truths = [S.rot_xy(0.01 * k, -0.015 * k, (0.01 * k, -0.005 * k, 0.015 * k)) for k in (1, 2, 3)]
    frames = [TS.live(pose=tuple(p))[0] for p in truths]
    tv = _volume()
    cam = cloud.Camera(S.W, S.H, S.CAM["fx"], S.CAM["fy"], S.CAM["cx"], S.CAM["cy"])
    dev = [_dev(m[None, None]) for m in frames[0]]
    img = torch.zeros((1, 3, S.H, S.W), dtype=torch.uint8, device="cuda")
    pbuf = _dev(IDENT)

    def run():
        P = pbuf.view(1, 3, 4)
        render = tv.raycast(cam, P[:, :, :3], P[:, :, 3], z_far=4.0, want_image=False, want_count=False)
        tv.track(*dev, render, poses=pbuf, H=S.H, W=S.W, **CAMERA, n_iters=6, min_count=6, max_rot=0.5, max_trans=0.5, want_systems=False)
        tv.integrate(*dev, img, poses=pbuf, **CAMERA, carve=True)

    run()                                                                      # the warm-up of the capture, on state that is reset below
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    tv.buffer.copy_(_dev(TS.volume()))
    pbuf.copy_(_dev(IDENT))
    vol, pose_o = TS.volume(), IDENT.copy()
    place = dict(**RS.place(TS.GRID))
    for k, maps in enumerate(frames):
        for d, m in zip(dev, maps):
            d.copy_(_dev(m[None, None]))
        before = pbuf.cpu().numpy()
        graph.replay()
        torch.cuda.synchronize()
        after = pbuf.cpu().numpy()
        # the oracle chain on the device's own input pose of this frame
        model = R.raycast(vol, before, **RS.CAM_OWN, **place, z_near=0.0, z_far=4.0, step=TS.GRID["trunc"] / 2)
        o = T.track(*[m[None] for m in maps], before, before, model["depth"], model["gradients"], n_iters=6, **TS.live()[1], **TS.model_kw(), **TS.GATES)
        pose_o = o["poses"]
        assert all(it["status"] == 0 for it in o["its"][0])
        assert np.abs(after - pose_o).max() < 1e-4                             # (six chained iterations: loose; the volume below is exact)
        vol, _ = O.integrate(vol, *[m[None] for m in maps], np.zeros((1, 3, S.H, S.W), np.uint8), after, **place, trunc=TS.GRID["trunc"],
                             max_weight=64, carve=True, **S.CAM)
        assert _bytes(tv.buffer.cpu().numpy()) == _bytes(vol), f"frame {k}"
    r0, t0 = T.pose_errors(S.IDENTITY, truths[-1])
    ro, to = T.pose_errors(pose_o[0], truths[-1])
    r1, t1 = T.pose_errors(after[0], truths[-1])
    print(f"[tsdf track loop] rotation {r0:.3g} -> {r1:.3g} (oracle {ro:.3g}), translation {t0:.3g} -> {t1:.3g} (oracle {to:.3g})")
    assert ro <= r0 / 5 and to <= t0 / 5                                       # of the oracle first
    assert r1 <= r0 / 5 and t1 <= t0 / 5


# ---- 8. the runner

def _s_model():
    from s2m2_amd.model import S2M2
    from s2m2_amd.spec import MODEL_CONFIGS
    from s2m2_amd.weights import seeded_state_dict
    C, ntr = MODEL_CONFIGS["S"]
    m = S2M2(C, 1, ntr, use_positivity=True, refine_iter=3)
    m.load_state_dict(seeded_state_dict(C, 1, ntr, 0), strict=True)
    return m.cuda().eval()


def test_runner_tracks_three_frames(hip, tmp_path):
    """s2m2_run_engine --tsdf-frames ... --tsdf-track --tsdf-poses-out: a plumbing test -- the written poses and statuses, the PLY and the printed
    "tsdf_tracked" / "tsdf_lost" equal what the Python path gives on the maps the same engine writes with --out, whatever the statuses are (a
    seeded model's disparity need not track)"""
    from s2m2_amd.build import RUNNER
    from s2m2_amd.export import export_engine
    from s2m2_amd.weights import synthetic_pair
    H, W = 384, 512
    calib_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bicycle2_calib.txt")
    c = cloud.read_calib_file(calib_path)
    cam = dict(fx=float(c["cam0"][0, 0]), fy=float(c["cam0"][1, 1]), cx=float(c["cam0"][0, 2]), cy=float(c["cam0"][1, 2]),
               baseline=float(c["baseline"]), doffs=float(c["doffs"]), depth_trunc=6.0, conf_min=0.02)
    engine = str(tmp_path / "s_384x512.s2m2")
    export_engine(_s_model(), engine, H, W)
    frames, lines = [], []
    for k, seed in enumerate((11, 11, 12)):                                    # the second frame repeats the first: it has something to track
        left, right = synthetic_pair(H, W, 1, 24, seed)
        u8 = left.clamp(0, 255).round().to(torch.uint8).contiguous()
        names = [str(tmp_path / f"{n}{k}") for n in ("left.f32", "right.f32", "image.u8")]
        for name, t in zip(names, (left.contiguous().numpy().astype("<f4"), right.contiguous().numpy().astype("<f4"), u8.numpy())):
            (tmp_path / name).write_bytes(t.tobytes())
        out = tmp_path / f"out{k}"
        out.mkdir()
        p = subprocess.run([RUNNER, engine, names[0], names[1], "--out", str(out)], capture_output=True, text=True, timeout=240)
        assert p.returncode == 0, p.stderr
        maps = [torch.from_numpy(np.fromfile(out / f"{n}.f32", dtype="<f4").reshape(1, 1, H, W)).cuda() for n in ("disp", "occ", "conf")]
        frames.append((maps, u8.cuda()))
        lines.append(" ".join(names + ([repr(float(x)) for x in S.IDENTITY] if k != 1 else [])))     # the second line comes without a pose
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    pc = cloud.reproject(*frames[0][0], frames[0][1], **cam)
    centre = pc.points(0).median(dim=0).values.cpu().numpy().astype(np.float64)
    dims, vs = (40, 32, 48), 0.02
    origin = [float(np.round(centre[a] - vs * dims[a] / 2, 2)) for a in range(3)]
    args = [RUNNER, engine, "--tsdf-frames", str(tmp_path / "list.txt"), "--tsdf-dims", ",".join(map(str, dims)), "--tsdf-voxel", str(vs),
            "--tsdf-origin", ",".join(repr(x) for x in origin), "--tsdf-trunc", "0.06", "--tsdf-carve", "--calib", calib_path,
            "--depth-trunc", "6", "--conf-min", "0.02", "--tsdf-ply", str(tmp_path / "t.ply"), "--tsdf-track", "--tsdf-track-iters", "4",
            "--tsdf-poses-out", str(tmp_path / "poses.txt")]
    p = subprocess.run(args, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr
    tv = cloud.TsdfVolume(dims, vs, origin, trunc=0.06, max_weight=32767)
    camera = cloud.Camera(W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    pose = np.array([S.IDENTITY], F)
    want, tracked, lost = [], 0, 0
    for k, (maps, image) in enumerate(frames):
        status = 0
        if k:
            q = pose.astype(np.float64).reshape(3, 4)
            render = tv.raycast(camera, q[:, :3], q[:, 3], want_image=False, want_count=False)
            tr = tv.track(*maps, render, poses=_dev(pose), **cam, n_iters=4)
            status = tr.status()
            if status == 0:
                pose = tr.poses.cpu().numpy()
            tracked, lost = tracked + (status == 0), lost + (status != 0)
        want.append((pose[0].copy(), status))
        if status == 0:
            tv.integrate(*maps, image, poses=_dev(pose), carve=True, **cam)
    surf = tv.extract()
    n = surf.size()
    print(f"[tsdf track runner] statuses {[s for _, s in want]}, {n} points")
    assert f'{{"tsdf_frames": 3, "tsdf_points": {n}, "tsdf_tracked": {tracked}, "tsdf_lost": {lost}}}' in p.stdout
    got = [line.split() for line in (tmp_path / "poses.txt").read_text().splitlines()]
    assert len(got) == 3 and all(len(g) == 13 for g in got)
    for g, (wp, ws) in zip(got, want):
        assert int(g[12]) == ws and _bytes(np.array([float(x) for x in g[:12]], F)) == _bytes(wp)
    assert n > 0 and cloud.read_ply_records(str(tmp_path / "t.ply")).tobytes() == surf.records[0, :n].cpu().numpy().tobytes()
