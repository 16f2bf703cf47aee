"""K24 on the GPU (include/s2m2_hip.h: s2m2_tsdf_integrate, s2m2_tsdf_extract; s2m2_amd/cloud.py: TsdfVolume) against the numpy oracle of
tests/tsdf_oracle.py -- never against the code under test.  Every comparison is an equality of bytes: the whole volume, every record and
gradient as int32 bits, and the count.  One thread owns a voxel and the points are ranked in voxel order, so nothing depends on timing.

Every scene asserts FROM THE ORACLE that it holds what it is meant to hold before anything is compared.  Voxels that no frame of a call
updates carry a sentinel pattern (a NaN tsdf, a negative weight) in the volume the call starts from; buffers the contract leaves untouched
are poisoned."""
import os
import subprocess

import numpy as np
import pytest
import torch

import tsdf_oracle as O
import tsdf_scenes as S
from s2m2_amd import cloud, utils

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = np.array([0x7fc00123, 0x80000001, 0xabcd1234, 0x5a5a9876], np.uint32).view(np.int32)     # NaN tsdf, weight < 0
ROT = S.rot_xy(0.1, -0.15, (0.05, -0.03, 0.1))
POSES3 = np.array([S.IDENTITY, ROT, S.IDENTITY], F)
KINDS3 = ["plane", "steps", "tilt"]


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()             # (a copy: the shared volumes are read-only)


def _place(grid):
    return dict(origin=grid["origin"], voxel_size=grid["voxel_size"])


def _gpu_integrate(hip, vol, frames, poses, grid, max_weight, carve, **over):
    disp, occ, conf, img = frames
    v = _dev(vol)
    hip.tsdf_integrate(v, _dev(disp[:, None]), _dev(occ[:, None]), _dev(conf[:, None]), _dev(img), _dev(np.asarray(poses, F)),
                       **{**S.CAM, **over}, **_place(grid), trunc=grid["trunc"], max_weight=max_weight, carve=carve)
    torch.cuda.synchronize()
    return v.cpu().numpy()


def _oracle_integrate(vol, frames, poses, grid, max_weight, carve):
    return O.integrate(vol, *frames, np.asarray(poses, F), **_place(grid), trunc=grid["trunc"], max_weight=max_weight, carve=carve, **S.CAM)


def _check_integrate(hip, frames, poses, grid, max_weight=64, carve=False, want=()):
    """one call from an empty volume whose never-updated voxels hold the sentinel; returns (oracle volume, diag).  want: skip classes that
    the scene must contain, besides UPDATED and one untouched voxel"""
    _, diag = _oracle_integrate(O.empty(grid["dims"]), frames, poses, grid, max_weight, carve)
    updated = np.any([d["cls"] == O.UPDATED for d in diag], axis=0)
    assert updated.any() and not updated.all()
    for c in want:
        assert any((d["cls"] == c).any() for d in diag), f"the scene has no voxel of skip class {c}"
    start = O.empty(grid["dims"])
    start.reshape(-1, 4)[~updated] = SENTINEL
    expect, diag = _oracle_integrate(start, frames, poses, grid, max_weight, carve)
    assert (expect.reshape(-1, 4)[~updated] == SENTINEL).all() and (expect.reshape(-1, 4)[updated, 1] > 0).all()
    got = _gpu_integrate(hip, start, frames, poses, grid, max_weight, carve)
    bad = np.flatnonzero((got != expect).reshape(-1, 4).any(1))
    assert got.tobytes() == expect.tobytes(), f"{len(bad)} voxels differ, first lin {bad[:5]}: {got.reshape(-1, 4)[bad[:2]]} vs {expect.reshape(-1, 4)[bad[:2]]}"
    return expect, diag


def _gpu_extract(hip, vol, grid, min_weight=1, capacity=None, records=True, gradients=True, count=True):
    """-> (records, gradients, count) as numpy, poisoned before the call (None where not requested)"""
    Nx, Ny, Nz = grid["dims"]
    cap = Nx * Ny * Nz if capacity is None else capacity
    rec = torch.full((cap, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if records else None
    grd = torch.full((cap, 3), float("nan"), dtype=torch.float32, device="cuda") if gradients else None
    cnt = torch.full((1,), -77, dtype=torch.int32, device="cuda") if count else None
    ws = torch.full((hip.tsdf_workspace_bytes(Nx, Ny, Nz),), 0xEE, dtype=torch.uint8, device="cuda")
    hip.tsdf_extract(_dev(vol), **_place(grid), min_weight=min_weight, workspace=ws, records=rec, gradients=grd, count=cnt)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (rec, grd, cnt))


def _check_extract(hip, vol, grid, min_weight=1, capacity=None, **which):
    e = O.extract(vol, **_place(grid), min_weight=min_weight)
    rec, grd, cnt = _gpu_extract(hip, vol, grid, min_weight, capacity, **which)
    n = e["count"]
    if cnt is not None:
        assert int(cnt[0]) == n
    for got, exp, poison in ((rec, e["records"], np.int32(0x5A5A5A5A)), (grd, e["gradients"], F("nan"))):
        if got is None:
            continue
        m = min(n, len(got))
        assert got[:m].view(np.int32).tobytes() == exp[:m].view(np.int32).tobytes()
        assert (got[m:].view(np.int32) == np.array(poison).view(np.int32)).all(), "stored beyond min(count, capacity)"
    return e


# ---- 1. awkward dims

@pytest.mark.parametrize("carve", [False, True])
@pytest.mark.parametrize("name", ["GRID_A", "GRID_ROW", "GRID_LONG"])
def test_awkward_dims(hip, name, carve):
    """dims that are no multiple of the 64 x 4 block or of the extraction tile; Nx = 1; a grid three tiles long"""
    grid = getattr(S, name)
    Nx, Ny, Nz = grid["dims"]
    tile = hip.tsdf_tile_voxels(Nx, Ny, Nz)
    assert Nx % 64 and Ny % 4 and (Nx * Ny * Nz) % tile
    if name == "GRID_LONG":
        assert Nx * Ny * Nz > 2 * tile
    vol, _ = _check_integrate(hip, S.frames(KINDS3), POSES3, grid, max_weight=2, carve=carve, want=(O.OUTSIDE, O.NOT_KEPT, O.BELOW_BAND))
    e = _check_extract(hip, vol, grid)
    assert e["count"] > 0 and (name == "GRID_ROW" or all((e["axis"] == a).any() for a in range(3)))
    assert name == "GRID_ROW" or e["far"].any() and not e["far"].all()


def test_crossings_across_a_tile_border(hip):
    """sign changes along x between the last voxel of a tile and the first of the next, and between the first two of a tile"""
    grid = S.GRID_LONG
    Nx, Ny, Nz = grid["dims"]
    tile = hip.tsdf_tile_voxels(Nx, Ny, Nz)
    vol, _ = _oracle_integrate(O.empty(grid["dims"]), S.frames(KINDS3), POSES3, grid, 8, False)
    v = vol.reshape(-1, 4)
    assert (tile - 1) % Nx < Nx - 2                                     # tile - 1, tile and tile + 1 are neighbours in one row
    for lin, t in ((tile - 1, -0.5), (tile, 0.5), (tile + 1, -0.25), (2 * tile - 1, 0.75), (2 * tile, -0.125)):
        v[lin] = [np.array(t, F).view(np.int32), 1, 0x40008000, 0xc000]
    e = O.extract(vol, **_place(grid))
    for lin in (tile - 1, tile, 2 * tile - 1):
        assert ((e["lin"] == lin) & (e["axis"] == 0)).any()
    _check_extract(hip, vol, grid)


# ---- 2. poses

BEHIND = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -2.0]              # Z = z - 2: half of the grid at Z <= 0, one slice at Z = 0 exactly


@pytest.mark.parametrize("pose", ["identity", "rotation", "behind", "wide"])
def test_poses(hip, pose):
    grid = S.GRID_DYADIC if pose == "behind" else S.GRID_A
    poses = dict(identity=[S.IDENTITY], rotation=[ROT], behind=[BEHIND], wide=[S.IDENTITY])[pose]
    carve = pose == "behind"                                   # the voxels in front of the camera are far in front of the plane
    want = dict(identity=(O.OUTSIDE,), rotation=(O.OUTSIDE, O.BELOW_BAND), behind=(O.BEHIND,), wide=(O.OUTSIDE,))[pose]
    _, diag = _check_integrate(hip, S.frames(["plane"]), poses, grid, carve=carve, want=want)
    d = diag[0]
    if pose == "behind":
        assert (d["Z"] == 0).any() and (d["Z"] < 0).any()
    if pose == "wide":                                         # the projection leaves the image on every side
        out = d["cls"] == O.OUTSIDE
        assert (d["fu"][out] < 0).any() and (d["fu"][out] >= S.W).any() and (d["fv"][out] < 0).any() and (d["fv"][out] >= S.H).any()


# ---- 3. rounding and band edges

@pytest.mark.parametrize("carve", [False, True])
def test_ties_band_edges_and_pixels_that_are_not_kept(hip, carve):
    grid = S.GRID_DYADIC
    frames = S.frames(["plane"])
    _, diag = _check_integrate(hip, frames, [S.IDENTITY], grid, carve=carve, want=(O.NOT_KEPT, O.BELOW_BAND))
    d = diag[0]
    seen = d["cls"] >= O.NOT_KEPT
    ties = np.concatenate([d[c][seen & (d[c] - np.floor(d[c]) == 0.5)] for c in ("up", "vp")])     # x.5 exactly: half to even goes both ways
    assert (np.rint(ties) > ties).any() and (np.rint(ties) < ties).any()
    tr = F(grid["trunc"])
    assert ((d["sdf"] == -tr) & (d["cls"] == O.UPDATED)).any() and ((d["sdf"] == tr) & (d["cls"] == O.UPDATED)).any()
    assert (d["cls"] == O.IN_FRONT).any() != carve             # sdf > trunc: skipped without carve, updated with it
    # among the pixels that are not kept: failed confidence, failed occlusion, NaN, +inf, -inf, zero and negative disparities
    disp, occ, conf, _ = frames
    import cloud_oracle
    under = d["pix"][d["cls"] == O.NOT_KEPT]
    dd, oo, cc = (cloud_oracle.crop(a[0], S.H, S.W).ravel()[under] for a in (disp, occ, conf))
    assert (cc < 0.1).any() and (oo <= 0.5).any() and np.isnan(dd).any() and (dd == np.inf).any() and (dd == -np.inf).any()
    assert (dd == 0).any() and (dd == -3).any()


# ---- 4. accumulation

def test_three_calls_of_one_frame_equal_one_call_of_three(hip):
    grid = S.GRID_A
    frames = S.frames(KINDS3, holes=False)
    expect, diag = _check_integrate(hip, frames, POSES3, grid, max_weight=5)
    times = np.sum([d["cls"] == O.UPDATED for d in diag], axis=0)
    assert (times == 3).any() and (times == 1).any()
    vol = O.empty(grid["dims"])
    vol.reshape(-1, 4)[times == 0] = SENTINEL
    for b in range(3):
        vol = _gpu_integrate(hip, vol, [a[b:b + 1] for a in frames], POSES3[b:b + 1], grid, 5, False)
    assert vol.tobytes() == expect.tobytes()


def test_weight_cap_and_colour_average(hip):
    """max_weight 2 with 4 frames of different colours: voxels sit at the cap and go on averaging"""
    grid = S.GRID_A
    frames = S.frames(["plane", "plane", "tilt", "plane"], holes=False)
    assert len({frames[3][b].tobytes() for b in range(4)}) == 4
    expect, diag = _check_integrate(hip, frames, [S.IDENTITY] * 4, grid, max_weight=2)
    times = np.sum([d["cls"] == O.UPDATED for d in diag], axis=0)
    u = O.unpack(expect)
    assert (times == 4).any() and (u["weight"][times >= 2] == 2).all() and (u["weight"][times == 1] == 1).all()
    assert (u["r"][times == 4] % 256 != 0).any()               # a real 8.8 average, not a byte


# ---- 5. image dtypes and map widths

@pytest.mark.parametrize("Hp,Wp", [(51, 73), (48, 80), (47, 70)])
@pytest.mark.parametrize("dtype", [np.uint8, np.float16, np.float32])
def test_image_dtypes_and_padded_widths(hip, dtype, Hp, Wp):
    frames = S.frames(["steps", "tilt"], Hp=Hp, Wp=Wp, dtype=dtype, seed=3)
    if dtype != np.uint8:
        img = frames[3].astype(np.float32)
        assert (img < 0).any() and (img > 255).any() and (np.abs(img - np.rint(img)) > 0.3).any()
    _check_integrate(hip, frames, [S.IDENTITY, ROT], S.GRID_A, carve=True)


# ---- 6. extraction

@pytest.fixture(scope="module")
def fused():
    """GRID_A after 3 frames that see all of it and 3 that see its left part only (weights 1 .. 6), with every eleventh voxel of a skewed
    lattice forgotten (weight 0 inside the band): the oracle's volume, shared and never changed"""
    vol = O.empty(S.GRID_A["dims"])
    aside = np.array(POSES3)
    aside[:, 3] += F(0.7)
    for seed, poses in ((0, POSES3), (1, aside)):
        vol, _ = _oracle_integrate(vol, S.frames(KINDS3, seed=seed), poses, S.GRID_A, 64, False)
    k, j, i = np.indices(vol.shape[:3])
    vol[..., 1][(i + 2 * j + 3 * k) % 11 == 0] = 0
    vol.setflags(write=False)
    return vol


@pytest.mark.parametrize("min_weight", [1, 3])
def test_extract_min_weight_and_gradients(hip, fused, min_weight):
    grid = S.GRID_A
    e = _check_extract(hip, fused, grid, min_weight=min_weight)
    w = O.unpack(fused)["weight"]
    assert e["count"] > 0 and ((w > 0) & (w < 3)).any() and (w >= 3).any()
    # gradients at the grid's faces and next to unobserved voxels: a point whose sel has a neighbour outside, and one whose sel has an
    # unobserved neighbour inside
    Nx, Ny, Nz = grid["dims"]
    sel = np.where(e["far"], e["lin"] + np.take((1, Nx, Nx * Ny), e["axis"]), e["lin"])
    i, j, k = sel % Nx, sel // Nx % Ny, sel // (Nx * Ny)
    assert ((i == 0) | (i == Nx - 1) | (j == 0) | (j == Ny - 1) | (k == 0) | (k == Nz - 1)).any()
    beside_unobserved = False
    for pos, extent, stride in ((i, Nx, 1), (j, Ny, Nx), (k, Nz, Nx * Ny)):
        inner = sel[(pos > 0) & (pos < extent - 1)]
        beside_unobserved |= bool((~e["observed"][inner + stride] | ~e["observed"][inner - stride]).any())
    assert beside_unobserved
    assert 0 < O.extract(fused, **_place(grid), min_weight=3)["count"] < O.extract(fused, **_place(grid), min_weight=1)["count"]


CAPACITY_CASES = [(c, w) for c in ("zero", "below", "above") for w in ("all", "no-gradients", "no-records", "no-count")
                  if (c, w) != ("zero", "no-count")]                 # capacity 0 leaves the count as the only output


@pytest.mark.parametrize("capacity,which", CAPACITY_CASES)
def test_extract_capacity(hip, fused, capacity, which):
    n = O.extract(fused, **_place(S.GRID_A))["count"]
    assert n > 20
    cap = dict(zero=0, below=n - 7, above=n + 9)[capacity]
    which = {"all": {}, "no-gradients": dict(gradients=False), "no-records": dict(records=False), "no-count": dict(count=False)}[which]
    _check_extract(hip, fused, S.GRID_A, capacity=cap, **which)


def test_a_tsdf_of_exactly_zero_gives_one_point(hip):
    grid = dict(dims=(7, 3, 2), origin=(0.0, 0.0, 0.0), voxel_size=0.5)
    vol = O.empty(grid["dims"])
    t = vol[..., 0].view(F)
    vol[..., 1] = 1
    t[...] = 0.25
    t[0, 0, :3] = [0.5, 0.0, -0.5]            # + 0 -: one point, at the voxel of the zero
    t[0, 1, 3:6] = [-0.5, 0.0, 0.5]           # - 0 +: one point, at the voxel of the zero
    t[1, 2, 4] = -0.0                         # a negative zero is not < 0
    t[0, 0, 3:] = -0.5
    e = _check_extract(hip, vol, grid)
    x_row0 = e["records"][(e["lin"] < 7) & (e["axis"] == 0)][:, 0].view(F)
    x_row1 = e["records"][(e["lin"] >= 7) & (e["lin"] < 14) & (e["axis"] == 0)][:, 0].view(F)
    assert x_row0.tolist() == [0.5] and 2.0 in x_row1.tolist() and (x_row1 == 2.0).sum() == 1


# ---- 7. reproducibility and graph replay

def test_two_runs_and_a_graph_replay_with_new_poses(hip):
    grid = S.GRID_A
    frames = S.frames(["steps", "tilt"], holes=False)
    poses = [np.array([S.IDENTITY, ROT], F), np.array([ROT, S.rot_xy(-0.05, 0.2, (0.0, 0.02, -0.1))], F)]
    expect, vol = [], O.empty(grid["dims"])
    for p in poses:
        vol, _ = _oracle_integrate(vol, frames, p, grid, 64, True)
        expect.append((vol, O.extract(vol, **_place(grid))))
    dev = [_dev(a[:, None]) for a in frames[:3]] + [_dev(frames[3])]
    Nx, Ny, Nz = grid["dims"]

    def run(v, pose_buf, out):
        hip.tsdf_integrate(v, *dev, pose_buf, **S.CAM, **_place(grid), trunc=grid["trunc"], max_weight=64, carve=True)
        hip.tsdf_extract(v, **_place(grid), workspace=out[3], records=out[0], gradients=out[1], count=out[2])

    def outputs():
        return (torch.zeros((Nx * Ny * Nz, 4), dtype=torch.int32, device="cuda"), torch.zeros((Nx * Ny * Nz, 3), dtype=torch.float32, device="cuda"),
                torch.zeros((1,), dtype=torch.int32, device="cuda"), torch.empty((hip.tsdf_workspace_bytes(Nx, Ny, Nz),), dtype=torch.uint8, device="cuda"))

    def same(v, out, step):
        torch.cuda.synchronize()
        vol, e = expect[step]
        n = e["count"]
        assert v.cpu().numpy().tobytes() == vol.tobytes() and int(out[2][0]) == n
        assert out[0][:n].cpu().numpy().tobytes() == e["records"].tobytes() and out[1][:n].cpu().numpy().view(np.int32).tobytes() == e["gradients"].view(np.int32).tobytes()

    for _ in range(2):                                         # two eager runs into fresh volumes (also the warm-up of the capture)
        v, out, buf = _dev(O.empty(grid["dims"])), outputs(), _dev(poses[0])
        for step, p in enumerate(poses):
            buf.copy_(_dev(p))
            run(v, buf, out)
            same(v, out, step)
    v, out, buf = _dev(O.empty(grid["dims"])), outputs(), _dev(poses[0])
    graph = torch.cuda.CUDAGraph()                             # (one stream, no side branches)
    with torch.cuda.graph(graph):
        run(v, buf, out)
    v.zero_()
    for step, p in enumerate(poses):                           # the pose buffer alone is rewritten between the replays
        buf.copy_(_dev(p))
        graph.replay()
        same(v, out, step)


# ---- 8. the Python layer

def test_tsdf_volume_end_to_end(hip, tmp_path):
    grid = S.GRID_A
    frames = S.frames(KINDS3)
    cam = {k: v for k, v in S.CAM.items() if k != "fy"}
    tv = cloud.TsdfVolume(grid["dims"], grid["voxel_size"], grid["origin"], trunc=grid["trunc"], max_weight=4)
    assert not tv.buffer.any() and tv.extract().size() == 0                                  # an all-zero volume is empty
    dev = [_dev(a[:, None]) for a in frames[:3]] + [_dev(frames[3])]
    tv.integrate(*dev, R=POSES3.reshape(3, 3, 4)[:, :, :3], t=POSES3.reshape(3, 3, 4)[:, :, 3], **cam)
    tv.integrate(*[a[:1] for a in dev], R=np.eye(3), t=[0.0, 0.0, 0.0], carve=True, **cam)
    vol, _ = _oracle_integrate(O.empty(grid["dims"]), frames, POSES3, grid, 4, False)
    vol, _ = _oracle_integrate(vol, [a[:1] for a in frames], [S.IDENTITY], grid, 4, True)
    assert tv.buffer.cpu().numpy().tobytes() == vol.tobytes()
    u = O.unpack(vol)
    assert tv.tsdf().cpu().numpy().ravel().view(np.int32).tobytes() == u["tsdf"].view(np.int32).tobytes()
    assert np.array_equal(tv.weight().cpu().numpy().ravel(), u["weight"])
    assert np.array_equal(tv.colour().cpu().numpy().reshape(-1, 3).astype(np.int64) & 0xffff, np.stack([u["r"], u["g"], u["b"]], 1))
    e = O.extract(vol, **_place(grid), min_weight=2)
    surf = tv.extract(min_weight=2)
    n = e["count"]
    assert n > 0 and surf.size() == n and surf.records[0, :n].cpu().numpy().tobytes() == e["records"].tobytes()
    assert surf.gradients().cpu().numpy().view(np.int32).tobytes() == e["gradients"].view(np.int32).tobytes()
    assert np.array_equal(surf.points().cpu().numpy(), e["records"][:, :3].view(F))
    nrm = surf.normals().cpu().numpy()
    nz = np.linalg.norm(e["gradients"], axis=1) > 0
    assert nz.any() and np.allclose(np.linalg.norm(nrm[nz], axis=1), 1.0, atol=1e-5)
    assert surf.write_ply(str(tmp_path / "s.ply")) == n
    assert cloud.read_ply_records(str(tmp_path / "s.ply")).tobytes() == e["records"].tobytes()
    assert surf.write_ply(str(tmp_path / "n.ply"), normals=True) == n
    raw = open(tmp_path / "n.ply", "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert b"property float nx" in head and f"element vertex {n}".encode() in head
    disk = np.frombuffer(body, dtype=cloud.NORMAL_RECORD_DTYPE)
    assert len(disk) == n and np.array_equal(disk["x"], e["records"][:, 0].view(F)) and np.array_equal(disk["nz"], nrm[:, 2])
    assert np.array_equal(disk["red"], e["records"][:, 3] & 0xff)
    assert tv.extract(capacity=5, want_gradients=False).size() == 5
    tv.reset()
    assert not tv.buffer.any()


def test_utils_integrate_tsdf(hip):
    """get_pointcloud's conventions: halved intrinsics, fx for both focal lengths, no confidence filter, depth_scale 1000"""
    disp, _, _, img = S.frames(["tilt"], Hp=S.H, Wp=S.W, holes=False)
    calib = dict(cam0=np.array([[128.0, 0, 67.0], [0, 128.0, 45.0], [0, 0, 1]]), baseline=1000.0, doffs=0.0)      # z = 64 / d metres
    grid = dict(dims=(9, 8, 21), origin=(-2.0, -2.0, 125.0), voxel_size=1.0, trunc=4.0)
    tv = cloud.TsdfVolume(grid["dims"], 1.0, grid["origin"])
    R, t = np.asarray(ROT).reshape(3, 4)[:, :3], [0.5, -0.25, 1.0]
    assert utils.integrate_tsdf(tv, img[0].transpose(1, 2, 0), disp[0], calib, R, t, depth_trunc=200.0) is tv
    cam = dict(fx=64.0, fy=64.0, cx=33.5, cy=22.5, baseline=1000.0, doffs=0.0, depth_scale=1000.0, depth_trunc=200.0, filtered=False)
    vol, diag = O.integrate(O.empty(grid["dims"]), disp, disp, disp, img, np.concatenate([R, np.array(t)[:, None]], 1).reshape(1, 12).astype(F),
                            **_place(grid), trunc=4.0, max_weight=64, **cam)
    assert (diag[0]["cls"] == O.UPDATED).sum() > 50
    assert tv.buffer.cpu().numpy().tobytes() == vol.tobytes()


# ---- 9. the runner

def _s_model():
    from s2m2_amd.model import S2M2
    from s2m2_amd.spec import MODEL_CONFIGS
    from s2m2_amd.weights import seeded_state_dict
    C, ntr = MODEL_CONFIGS["S"]
    m = S2M2(C, 1, ntr, use_positivity=True, refine_iter=3)
    m.load_state_dict(seeded_state_dict(C, 1, ntr, 0), strict=True)
    return m.cuda().eval()


def test_runner_fuses_two_frames(hip, tmp_path):
    """s2m2_run_engine --tsdf-frames: the PLY equals what TsdfVolume gives on the maps the same engine writes with --out"""
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
    poses = [S.IDENTITY, [1, 0, 0, 0.03125, 0, 1, 0, -0.015625, 0, 0, 1, 0.0625]]      # (dyadic: one value as text, float and double)
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
    (tmp_path / "list.txt").write_text("# left right image pose\n" + "\n".join(lines) + "\n")
    # a grid around the first frame's median point
    pc = cloud.reproject(*frames[0][0], frames[0][1], **cam)
    centre = pc.points(0).median(dim=0).values.cpu().numpy().astype(np.float64)
    dims, vs = (40, 32, 48), 0.02
    origin = [float(np.round(centre[a] - vs * dims[a] / 2, 2)) for a in range(3)]
    p = subprocess.run([RUNNER, engine, "--tsdf-frames", str(tmp_path / "list.txt"), "--tsdf-dims", ",".join(map(str, dims)), "--tsdf-voxel", str(vs),
                        "--tsdf-origin", ",".join(repr(x) for x in origin), "--tsdf-trunc", "0.06", "--tsdf-carve", "--calib", calib_path,
                        "--depth-trunc", "6", "--conf-min", "0.02", "--tsdf-ply", str(tmp_path / "t.ply")], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr
    tv = cloud.TsdfVolume(dims, vs, origin, trunc=0.06, max_weight=32767)
    for (maps, image), pose in zip(frames, poses):
        q = np.asarray(pose, np.float64).reshape(3, 4)
        tv.integrate(*maps, image, R=q[:, :3], t=q[:, 3], carve=True, **cam)
    surf = tv.extract()
    n = surf.size()
    print(f"[tsdf runner] {n} points, {int((tv.weight() > 0).sum())} voxels updated")
    assert n > 0 and f'"tsdf_points": {n}' in p.stdout and '"tsdf_frames": 2' in p.stdout
    assert cloud.read_ply_records(str(tmp_path / "t.ply")).tobytes() == surf.records[0, :n].cpu().numpy().tobytes()
