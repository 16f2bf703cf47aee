"""K26 on the GPU (include/s2m2_hip.h: s2m2_tsdf_raycast; s2m2_amd/cloud.py: TsdfVolume.raycast) against the numpy oracle of
tests/tsdf_raycast_oracle.py -- never against the code under test.  Every comparison is an equality of bytes: depth and gradients as int32
bits, the image and the count.  One thread owns a pixel and the count is a sum of integers, so nothing depends on timing.

Every scene asserts FROM THE ORACLE that it holds what it is meant to hold before anything is compared.  All four outputs are allocated and
poisoned before each call, each with a guard behind it; the guards, and the outputs that a call does not request, must still hold the poison."""
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
from s2m2_amd import cloud, utils

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64
POISON = dict(depth=0x7fc00123, gradients=0x7fc00456, image=0xA5, count=-77)
DTYPE = dict(depth=torch.int32, gradients=torch.int32, image=torch.uint8, count=torch.int32)     # float outputs are poisoned as bits
ALL = ("depth", "gradients", "image", "count")


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


@pytest.fixture(scope="module")
def fused():
    """the fused grids, computed once and never changed: name -> volume"""
    return {name: RS.fuse(getattr(S, name), max_weight=2) for name in ("GRID_A", "GRID_DYADIC", "GRID_LONG", "GRID_ROW")}


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _shape(key, B, Ht, Wt):
    return dict(depth=(B, 1, Ht, Wt), gradients=(B, 3, Ht, Wt), image=(B, 3, Ht, Wt), count=(B,))[key]


def _gpu(hip, vol, poses, which=ALL, **args):
    """one call -> the requested outputs as numpy; the guards and the outputs not requested are checked for their poison here"""
    B, Ht, Wt = len(poses), args["Ht"], args["Wt"]
    flat, view = {}, {}
    for key in ALL:
        n = int(np.prod(_shape(key, B, Ht, Wt)))
        flat[key] = torch.full((n + GUARD,), POISON[key], dtype=DTYPE[key], device="cuda")
        v = flat[key][:n].view(_shape(key, B, Ht, Wt))
        view[key] = v.view(torch.float32) if key in ("depth", "gradients") else v
    hip.tsdf_raycast(_dev(vol), _dev(np.asarray(poses, F)), **args, **{k: view[k] for k in which})
    torch.cuda.synchronize()
    for key in ALL:
        n = int(np.prod(_shape(key, B, Ht, Wt)))
        assert (flat[key][n:] == POISON[key]).all(), f"written behind {key}"
        if key not in which:
            assert (flat[key] == POISON[key]).all(), f"{key} was not requested"
    return {k: view[k].cpu().numpy() for k in which}


def _same(got, r, what=""):
    for key, g in got.items():
        e = r[key]
        if key in ("depth", "gradients"):
            bad = np.argwhere(g.view(np.int32) != e.view(np.int32))
            assert g.view(np.int32).tobytes() == e.view(np.int32).tobytes(), f"{what} {key}: {len(bad)} differ, first {bad[:3].tolist()}: " \
                f"{[g[tuple(i)] for i in bad[:3]]} vs {[e[tuple(i)] for i in bad[:3]]}"
        else:
            assert g.tobytes() == e.tobytes(), f"{what} {key}: {np.argwhere(g != e)[:3].tolist()}"


def _check(hip, vol, poses, which=ALL, **args):
    """one K26 call against the oracle -> the oracle's dict"""
    r = R.raycast(vol, np.asarray(poses, F), **args)
    print(f"[tsdf raycast] {args['Ht']}x{args['Wt']} steps {r['n_steps']}: covered {r['count'].tolist()}")
    _same(_gpu(hip, vol, poses, which, **args), r)
    return r


# ---- 1. fused grids

@pytest.mark.parametrize("cam", ["CAM_ODD", "CAM_OWN"])
@pytest.mark.parametrize("name", ["GRID_A", "GRID_DYADIC", "GRID_LONG"])
def test_fused_grids(hip, fused, name, cam):
    """three poses in one call: where the frames were taken, rotated and moved, and looking away from the grid"""
    grid, cam = getattr(S, name), getattr(RS, cam)
    r = _check(hip, fused[name], RS.POSES3, **cam, **RS.place(grid), **RS.march(grid))
    n = cam["Ht"] * cam["Wt"]
    assert 0 < r["count"][0] < n and 0 < r["count"][1] < n
    assert r["count"][2] == 0 and not r["depth"][2].any() and not r["gradients"][2].any() and not r["image"][2].any()


# ---- 2. random volumes

@pytest.mark.parametrize("unobserved", [0.0, 0.1])
def test_random_volumes(hip, unobserved):
    g = RS.RANDOM_GRID
    assert g["dims"] == (20, 19, 18)
    vol = RS.random_volume(g["dims"], 5, unobserved)
    r = _check(hip, vol, RS.POSES3[:2], **RS.CAM_ODD, **RS.place(g), **RS.march(g, step=0.03))
    share = r["count"].sum() / (2 * RS.CAM_ODD["Ht"] * RS.CAM_ODD["Wt"])
    assert 0 < share < 1
    assert ((r["steps"] >= 2) & (r["depth"][:, 0] > 0)).any()
    if unobserved:
        assert (r["reset"] & (r["depth"][:, 0] > 0)).any(), "no ray hits behind a reset of have_prev"
        assert r["hit_unobserved"].any() and not r["depth"][:, 0][r["hit_unobserved"]].any(), "no ray ends in an unobserved hit sample"


# ---- 3. ties

@pytest.mark.parametrize("z_near,step", [(0.0, 0.125), (0.0625, 0.125), (0.0, 0.0625)])
def test_ties(hip, z_near, step):
    """dyadic numbers throughout: samples on voxel centres and on g == N - 1, tsdf values of exactly +0.0 and -0.0 in front of a crossing, a hit
    half way between two centres"""
    r = _check(hip, RS.ties_volume(), RS.TIES_POSES, **RS.TIES_CAM, **RS.place(RS.TIES_GRID), z_near=z_near, z_far=2.25, step=step)
    tp = r["t_prev"]
    if z_near == 0.0:
        assert r["on_centre"][:, 4, 4].all() and r["on_edge"][0, 4, 4] and r["steps"][0, 4, 4] == -1 and r["depth"][0, 0, 4, 4] == 0
        assert tp[1, 4, 4] == 0 and not np.signbit(tp[1, 4, 4]) and tp[2, 4, 4] == 0 and np.signbit(tp[2, 4, 4])
        assert r["depth"][1, 0, 4, 4] == F(1.25) and r["depth"][2, 0, 4, 4] == F(1.25) and (r["fr_hit"][1:, :, 4, 4] == 0).all()
    else:
        assert r["fr_hit"][2, 2, 4, 4] == F(0.5) and (r["fr_hit"][2, :2, 4, 4] == 0).all()
        k0 = int((r["depth"][2, 0, 4, 4] - 1.0) / 0.125)                    # the colour is the voxel's behind the hit
        assert r["image"][2, 0, 4, 4] == ((int(RS.ties_volume()[k0 + 1, 4, 8, 2]) & 0xffff) + 128) >> 8


# ---- 4. an extent of 1

def test_a_grid_with_an_extent_of_one_is_all_holes(hip, fused):
    grid = S.GRID_ROW
    assert grid["dims"][0] == 1 and (O.unpack(fused["GRID_ROW"])["weight"] > 0).any()
    r = _check(hip, fused["GRID_ROW"], RS.POSES3[:2], **RS.CAM_OWN, **RS.place(grid), **RS.march(grid))
    assert not r["count"].any() and not r["depth"].any()


# ---- 5. non-finite poses

def test_non_finite_poses_are_all_holes(hip, fused):
    """the float comparisons of the OBSERVED predicate come before any conversion to int: a NaN or Inf position forms no address"""
    grid = S.GRID_A
    nan_row, inf_t, ninf_t, nan_r, inf_r = (np.array(S.IDENTITY, F) for _ in range(5))
    nan_row[:] = np.nan
    inf_t[3] = np.inf
    ninf_t[11] = -np.inf
    nan_r[5] = np.nan
    inf_r[10] = np.inf
    poses = np.stack([nan_row, np.array(RS.ROT, F), inf_t, ninf_t, nan_r, inf_r, np.full(12, np.inf, F), np.full(12, -np.inf, F)])
    r = _check(hip, fused["GRID_A"], poses, **RS.CAM_ODD, **RS.place(grid), **RS.march(grid))
    assert r["count"][1] > 0 and not np.delete(r["count"], 1).any() and not np.delete(r["depth"], 1, axis=0).any()


# ---- 6. range and step

def _dyadic_plane():
    g = S.GRID_DYADIC
    vol, _ = O.integrate(O.empty(g["dims"]), *S.frames(["plane"], holes=False), np.array([S.IDENTITY], F), **RS.place(g), trunc=g["trunc"],
                         max_weight=64, **S.CAM)
    return g, vol


def test_z_far_just_before_and_just_behind_the_surface(hip):
    """the plane at z = 2 with samples every 1/8: the sample at 2 is exactly 0.0, not negative; the crossing needs the one at 2.125"""
    g, vol = _dyadic_plane()
    args = dict(**RS.CAM_OWN, **RS.place(g), z_near=0.0, step=0.125)
    before = _check(hip, vol, [S.IDENTITY], z_far=2.125, **args)
    behind = _check(hip, vol, [S.IDENTITY], z_far=2.126, **args)
    assert before["n_steps"] == 17 and behind["n_steps"] == 18 and before["count"][0] == 0 and behind["count"][0] > 0
    assert (behind["depth"][behind["depth"] != 0] == F(2.0)).all()


def test_step_above_the_band_and_z_near_inside_it(hip, fused):
    grid = S.GRID_A
    vol = fused["GRID_A"]
    fine = R.raycast(vol, RS.POSES3[:2], **RS.CAM_ODD, **RS.place(grid), **RS.march(grid))
    coarse = _check(hip, vol, RS.POSES3[:2], **RS.CAM_ODD, **RS.place(grid), **RS.march(grid, step=0.75))
    assert 2 * grid["trunc"] < 0.75 and coarse["count"].sum() < fine["count"].sum()              # the oracle says what a coarse march misses
    inside = _check(hip, vol, RS.POSES3[:2], **RS.CAM_ODD, **RS.place(grid), **RS.march(grid, z_near=1.9))
    assert 0 < inside["count"].sum() and (inside["depth"] != fine["depth"]).any()


def test_min_weight(hip):
    grid = S.GRID_A
    vol = RS.fuse(grid, max_weight=64)
    assert O.unpack(vol)["weight"].max() == 3
    one = _check(hip, vol, RS.POSES3[:2], **RS.CAM_ODD, **RS.place(grid), **RS.march(grid), min_weight=1)
    three = _check(hip, vol, RS.POSES3[:2], **RS.CAM_ODD, **RS.place(grid), **RS.march(grid), min_weight=3)
    assert 0 < three["count"].sum() < one["count"].sum()


def test_a_camera_far_away(hip, fused):
    """a thousand units from the grid a position in voxel units has ulps of 1e-3 voxel, and all but thirty of seven hundred samples lie outside
    the grid: what the kernel skips there must be what the rule calls unobserved"""
    grid = S.GRID_A
    c, back = np.array([0.0, 0.0, 2.0]), np.array([0.0, 0.0, 1000.0])
    poses = []
    for ax, ay in ((0.0, 0.0), (0.02, -0.03)):                              # turned about the grid's middle, then moved back
        Rm = np.asarray(S.rot_xy(ax, ay, (0, 0, 0))).reshape(3, 4)[:, :3]
        poses.append(np.concatenate([Rm, (c + back - Rm @ c)[:, None]], 1).ravel())
    cam = dict(Ht=37, Wt=53, fx=15000.0, fy=15000.0, cx=26.2, cy=18.1)
    r = _check(hip, fused["GRID_A"], poses, **cam, **RS.place(grid), z_near=900.0, z_far=1004.0, step=0.15)
    assert r["n_steps"] == 694 and (r["count"] > 100).all() and (r["steps"][r["steps"] >= 0] > 660).all()


# ---- 7. target tiling

@pytest.mark.parametrize("Ht,Wt", [(37, 1), (1, 53), (17, 65), (8, 32)])
def test_target_tiling(hip, fused, Ht, Wt):
    """one column, one row, one pixel more than two 32-pixel blocks in x with rows that are no multiple of the 8 of a patch, exactly one block"""
    grid = S.GRID_A
    cam = dict(Ht=Ht, Wt=Wt, fx=41.3 * max(Wt, 8) / 53, fy=39.7 * max(Ht, 8) / 37, cx=(Wt - 1) / 2 + 0.3, cy=(Ht - 1) / 2 - 0.2)
    r = _check(hip, fused["GRID_A"], RS.POSES3, **cam, **RS.place(grid), **RS.march(grid))
    assert r["count"][:2].sum() > 0


# ---- 8. outputs

@pytest.mark.parametrize("which", [c for n in range(1, 5) for c in itertools.combinations(ALL, n)], ids="-".join)
def test_every_subset_of_the_outputs(hip, fused, which):
    grid = S.GRID_A
    r = _check(hip, fused["GRID_A"], RS.POSES3[:2], which, **RS.CAM_ODD, **RS.place(grid), **RS.march(grid))
    assert r["count"].sum() > 0


def test_no_output_is_an_error(hip, fused):
    grid = S.GRID_A
    with pytest.raises(ValueError, match="no output requested"):
        hip.tsdf_raycast(_dev(fused["GRID_A"]), _dev(RS.POSES3), **RS.CAM_ODD, **RS.place(grid), **RS.march(grid))


# ---- 9. two runs and a graph replay

def test_two_runs_and_a_graph_replay_after_a_further_integrate(hip):
    """integrate + raycast captured once; between the replays only the two pose buffers are rewritten"""
    grid = S.GRID_A
    frames = S.frames(["steps", "tilt"], holes=False)
    fuse_poses = [np.array([S.IDENTITY, RS.ROT], F), np.array([RS.ROT, S.rot_xy(-0.05, 0.2, (0.0, 0.02, -0.1))], F)]
    view_poses = [np.array([S.IDENTITY, RS.ROT], F), np.array([S.rot_xy(0.05, 0.1, (-0.05, 0.0, 0.05)), S.IDENTITY], F)]
    args = dict(**RS.CAM_ODD, **RS.place(grid), **RS.march(grid))
    expect, vol = [], O.empty(grid["dims"])
    for fp, vp in zip(fuse_poses, view_poses):
        vol, _ = O.integrate(vol, *frames, fp, **RS.place(grid), trunc=grid["trunc"], max_weight=64, carve=True, **S.CAM)
        expect.append((vol, R.raycast(vol, vp, **args)))
    assert all(e["count"].sum() > 0 for _, e in expect) and expect[0][1]["depth"].tobytes() != expect[1][1]["depth"].tobytes()
    dev = [_dev(a[:, None]) for a in frames[:3]] + [_dev(frames[3])]
    Ht, Wt = args["Ht"], args["Wt"]

    def outputs():
        return dict(depth=torch.full((2, 1, Ht, Wt), -1.0, device="cuda"), gradients=torch.full((2, 3, Ht, Wt), -1.0, device="cuda"),
                    image=torch.full((2, 3, Ht, Wt), 7, dtype=torch.uint8, device="cuda"), count=torch.full((2,), -5, dtype=torch.int32, device="cuda"))

    def run(v, fuse_buf, view_buf, out):
        hip.tsdf_integrate(v, *dev, fuse_buf, **S.CAM, **RS.place(grid), trunc=grid["trunc"], max_weight=64, carve=True)
        hip.tsdf_raycast(v, view_buf, **args, **out)

    def same(v, out, step):
        torch.cuda.synchronize()
        vol, e = expect[step]
        assert v.cpu().numpy().tobytes() == vol.tobytes()
        _same({k: t.cpu().numpy() for k, t in out.items()}, e, f"step {step}")

    for _ in range(2):                                         # two eager runs into fresh volumes (also the warm-up of the capture)
        v, out, fb, vb = _dev(O.empty(grid["dims"])), outputs(), _dev(fuse_poses[0]), _dev(view_poses[0])
        for step in range(2):
            fb.copy_(_dev(fuse_poses[step]))
            vb.copy_(_dev(view_poses[step]))
            run(v, fb, vb, out)
            same(v, out, step)
    v, out, fb, vb = _dev(O.empty(grid["dims"])), outputs(), _dev(fuse_poses[0]), _dev(view_poses[0])
    graph = torch.cuda.CUDAGraph()                             # (one stream, no side branches)
    with torch.cuda.graph(graph):
        run(v, fb, vb, out)
    v.zero_()
    for step in range(2):
        fb.copy_(_dev(fuse_poses[step]))
        vb.copy_(_dev(view_poses[step]))
        graph.replay()
        same(v, out, step)


# ---- 10. the Python layer

def _far_corner(grid, poses):
    """the largest distance from a camera centre to a corner of the grid, in double"""
    ext = (np.array(grid["dims"], np.float64) - 1) * grid["voxel_size"]
    corners = np.array(grid["origin"])[None] + np.array(list(itertools.product((0, 1), repeat=3)), np.float64) * ext[None]
    q = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    centres = -np.einsum("bji,bj->bi", q[:, :, :3], q[:, :, 3])
    return float(np.linalg.norm(corners[None] - centres[:, None], axis=2).max())


def test_tsdf_volume_raycast_end_to_end(hip, fused):
    grid = S.GRID_A
    tv = cloud.TsdfVolume(grid["dims"], grid["voxel_size"], grid["origin"], trunc=grid["trunc"])
    tv.buffer.copy_(_dev(fused["GRID_A"]))
    q = RS.POSES3.astype(np.float64).reshape(3, 3, 4)
    camera = cloud.Camera(RS.CAM_ODD["Wt"], RS.CAM_ODD["Ht"], *(RS.CAM_ODD[k] for k in ("fx", "fy", "cx", "cy")), R=q[1, :, :3], t=q[1, :, 3])
    # the defaults: the camera's own pose, step = trunc / 2, z_far = the farthest corner, all outputs
    one = tv.raycast(camera)
    e = R.raycast(fused["GRID_A"], RS.POSES3[1:2], **RS.CAM_ODD, **RS.place(grid), z_near=0.0, z_far=_far_corner(grid, RS.POSES3[1:2]),
                  step=grid["trunc"] / 2)
    _same(dict(depth=one.depth.cpu().numpy(), gradients=one.gradients_buf.cpu().numpy(), image=one.image.cpu().numpy(), count=one.count.cpu().numpy()), e)
    n = RS.CAM_ODD["Ht"] * RS.CAM_ODD["Wt"]
    assert 0 < e["count"][0] < n and one.holes() == n - e["count"][0]
    # three poses, a range and a step of the caller's, no image
    r = tv.raycast(camera, R=q[:, :, :3], t=torch.from_numpy(q[:, :, 3]).cuda(), min_weight=2, z_near=1.0, z_far=3.5, step=0.07, want_image=False)
    e = R.raycast(fused["GRID_A"], RS.POSES3, **RS.CAM_ODD, **RS.place(grid), min_weight=2, z_near=1.0, z_far=3.5, step=0.07)
    assert r.image is None and tuple(r.depth.shape) == (3, 1, 37, 53)
    _same(dict(depth=r.depth.cpu().numpy(), gradients=r.gradients_buf.cpu().numpy(), count=r.count.cpu().numpy()), e)
    assert [r.holes(b) for b in range(3)] == [n - c for c in e["count"]] and r.holes(2) == n
    nrm = r.normals().cpu().numpy()
    covered = e["depth"][:, 0] != 0
    assert np.allclose(np.linalg.norm(nrm, axis=1)[covered], 1.0, atol=1e-5) and not nrm.transpose(0, 2, 3, 1)[~covered].any()
    assert (nrm[:, 2][covered] < 0).all()                                  # towards the camera
    bare = tv.raycast(camera, want_gradients=False, want_image=False, want_count=False)
    assert bare.gradients_buf is None and bare.image is None and bare.count is None and bare.depth.cpu().numpy().tobytes() == one.depth.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="want_gradients=False"):
        bare.normals()
    with pytest.raises(ValueError, match="want_count=False"):
        bare.holes()
    with pytest.raises(ValueError, match=r"R is \(3,3\) or \(1,3,3\)"):
        tv.raycast(camera, R=np.eye(2), t=np.zeros(3))
    with pytest.raises(ValueError, match="at most 65536"):
        tv.raycast(camera, step=1e-6)
    with pytest.raises(ValueError, match="z_near < z_far"):
        tv.raycast(camera, z_near=5.0, z_far=4.0)
    with pytest.raises(ValueError, match="min_weight"):
        tv.raycast(camera, min_weight=0)


def test_normals_of_the_dyadic_plane_are_exact(hip):
    """Gx == Gy == 0 exactly, so the normalised camera-frame normal is (0, 0, -1) to the bit"""
    g, vol = _dyadic_plane()
    tv = cloud.TsdfVolume(g["dims"], g["voxel_size"], g["origin"], trunc=g["trunc"])
    tv.buffer.copy_(_dev(vol))
    r = tv.raycast(cloud.Camera(S.W, S.H, S.CAM["fx"], S.CAM["fy"], S.CAM["cx"], S.CAM["cy"]))
    covered = (r.depth[0, 0] != 0).cpu().numpy()
    assert covered.sum() == r.depth.numel() - r.holes() > 0 and (r.depth[0, 0].cpu().numpy()[covered] == F(2.0)).all()
    nrm = r.normals()[0].cpu().numpy()
    assert (nrm[0][covered] == 0).all() and (nrm[1][covered] == 0).all() and (nrm[2][covered] == -1).all() and not nrm[:, ~covered].any()


def test_utils_render_tsdf(hip):
    """get_pointcloud's conventions: halved intrinsics, fx for both focal lengths; the size from the calibration or from the caller"""
    g, vol = _dyadic_plane()
    tv = cloud.TsdfVolume(g["dims"], g["voxel_size"], g["origin"], trunc=g["trunc"])
    tv.buffer.copy_(_dev(vol))
    calib = dict(cam0=np.array([[128.0, 0, 67.0], [0, 120.0, 45.0], [0, 0, 1]]), width=2 * S.W, height=2 * S.H)
    q = np.asarray(RS.ROT, np.float64).reshape(3, 4)
    r = utils.render_tsdf(tv, calib, q[:, :3], q[:, 3])
    args = dict(fx=64.0, fy=64.0, cx=33.5, cy=22.5, **RS.place(g), z_near=0.0, z_far=_far_corner(g, [RS.ROT]), step=g["trunc"] / 2)
    e = R.raycast(vol, np.array([RS.ROT], F), Ht=S.H, Wt=S.W, **args)
    assert isinstance(r, cloud.TsdfRender) and e["count"][0] > 0
    _same(dict(depth=r.depth.cpu().numpy(), gradients=r.gradients_buf.cpu().numpy(), image=r.image.cpu().numpy(), count=r.count.cpu().numpy()), e)
    r = utils.render_tsdf(tv, calib, q[:, :3], q[:, 3], size=(40, 30))
    e = R.raycast(vol, np.array([RS.ROT], F), Ht=30, Wt=40, **args)
    _same(dict(depth=r.depth.cpu().numpy(), count=r.count.cpu().numpy()), e)


# ---- 11. the runner

def _s_model():
    from s2m2_amd.model import S2M2
    from s2m2_amd.spec import MODEL_CONFIGS
    from s2m2_amd.weights import seeded_state_dict
    C, ntr = MODEL_CONFIGS["S"]
    m = S2M2(C, 1, ntr, use_positivity=True, refine_iter=3)
    m.load_state_dict(seeded_state_dict(C, 1, ntr, 0), strict=True)
    return m.cuda().eval()


def test_runner_renders_two_frames(hip, tmp_path):
    """s2m2_run_engine --tsdf-frames ... --tsdf-render: the written depth and image equal what TsdfVolume.raycast gives on the volume rebuilt
    from the maps the same engine writes with --out, and "tsdf_render_pixels" joins the printed line"""
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
    poses = [S.IDENTITY, [1, 0, 0, 0.03125, 0, 1, 0, -0.015625, 0, 0, 1, 0.0625]]
    frames, lines = [], []
    for k, seed in enumerate((11, 12)):
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
        lines.append(" ".join(names + [repr(float(x)) for x in poses[k]]))
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    pc = cloud.reproject(*frames[0][0], frames[0][1], **cam)
    centre = pc.points(0).median(dim=0).values.cpu().numpy().astype(np.float64)
    dims, vs = (40, 32, 48), 0.02
    origin = [float(np.round(centre[a] - vs * dims[a] / 2, 2)) for a in range(3)]
    args = [RUNNER, engine, "--tsdf-frames", str(tmp_path / "list.txt"), "--tsdf-dims", ",".join(map(str, dims)), "--tsdf-voxel", str(vs),
            "--tsdf-origin", ",".join(repr(x) for x in origin), "--tsdf-trunc", "0.06", "--tsdf-carve", "--calib", calib_path,
            "--depth-trunc", "6", "--conf-min", "0.02", "--tsdf-ply", str(tmp_path / "t.ply"),
            "--tsdf-render", ",".join(repr(float(x)) for x in poses[0]), "--tsdf-render-depth", str(tmp_path / "d.f32"),
            "--tsdf-render-image", str(tmp_path / "i.u8")]
    p = subprocess.run(args, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr
    tv = cloud.TsdfVolume(dims, vs, origin, trunc=0.06, max_weight=32767)
    for (maps, image), pose in zip(frames, poses):
        q = np.asarray(pose, np.float64).reshape(3, 4)
        tv.integrate(*maps, image, R=q[:, :3], t=q[:, 3], carve=True, **cam)
    q = np.asarray(poses[0], np.float64).reshape(3, 4)
    r = tv.raycast(cloud.Camera(W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"]), R=q[:, :3], t=q[:, 3])
    n, pixels = tv.extract().size(), int(r.count[0].item())
    print(f"[tsdf raycast runner] {n} points, {pixels} of {H * W} pixels covered")
    assert 0 < pixels < H * W
    assert f'{{"tsdf_frames": 2, "tsdf_points": {n}, "tsdf_render_pixels": {pixels}}}' in p.stdout
    assert np.fromfile(tmp_path / "d.f32", dtype="<f4").view(np.int32).tobytes() == r.depth.cpu().numpy().view(np.int32).tobytes()
    assert (tmp_path / "i.u8").read_bytes() == r.image.cpu().numpy().tobytes()
