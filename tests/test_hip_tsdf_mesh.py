"""K25 on the GPU (include/s2m2_hip.h: s2m2_tsdf_mesh; s2m2_amd/cloud.py: TsdfVolume.extract_mesh) against the numpy oracle of
tests/tsdf_mesh_oracle.py -- never against the code under test.  Every comparison is an equality: the faces as int32, the face count, and the
vertices (records, gradients, count) byte for byte, against the oracle AND against an s2m2_tsdf_extract run on the same volume.  The workspace and
every output buffer are poisoned before each call, and what the contract leaves untouched must still hold the poison.

Every scene asserts FROM THE ORACLE that it holds what it is meant to hold before anything is compared."""
import os
import subprocess

import numpy as np
import pytest
import torch

import tsdf_mesh_oracle as M
import tsdf_oracle as O
import tsdf_scenes as S
from s2m2_amd import cloud

pytestmark = pytest.mark.gpu

F = np.float32
ROT = S.rot_xy(0.1, -0.15, (0.05, -0.03, 0.1))
POSES3 = np.array([S.IDENTITY, ROT, S.IDENTITY], F)
KINDS3 = ["plane", "steps", "tilt"]
REC_POISON, FACE_POISON = 0x5A5A5A5A, 0x3C3C3C3C


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _place(grid):
    return dict(origin=grid["origin"], voxel_size=grid["voxel_size"])


def _grid(dims):
    return dict(dims=dims, origin=(-0.4, 0.3, 1.25), voxel_size=0.05, trunc=0.2)


def _fuse(grid, kinds=KINDS3, poses=POSES3, max_weight=64, seed=0):
    vol, _ = O.integrate(O.empty(grid["dims"]), *S.frames(kinds, seed=seed), np.asarray(poses, F), **_place(grid), trunc=grid["trunc"],
                         max_weight=max_weight, **S.CAM)
    return vol


def _random_volume(dims, seed, unobserved=0.0):
    """random signs and magnitudes written straight into the buffer, colours that differ from voxel to voxel"""
    g = np.random.default_rng(seed)
    Nx, Ny, Nz = dims
    vol = O.empty(dims)
    vol[..., 0] = g.uniform(-1, 1, (Nz, Ny, Nx)).astype(F).view(np.int32)
    vol[..., 1] = np.where(g.random((Nz, Ny, Nx)) < unobserved, 0, g.integers(1, 5, (Nz, Ny, Nx)))
    vol[..., 2] = g.integers(0, 65281, (Nz, Ny, Nx)) | g.integers(0, 65281, (Nz, Ny, Nx)) << 16
    vol[..., 3] = g.integers(0, 65281, (Nz, Ny, Nx))
    return vol


def _buffers(cap, fcap, records=True, gradients=True, count=True, faces=True):
    return dict(records=torch.full((cap, 4), REC_POISON, dtype=torch.int32, device="cuda") if records else None,
                gradients=torch.full((cap, 3), float("nan"), dtype=torch.float32, device="cuda") if gradients else None,
                count=torch.full((1,), -77, dtype=torch.int32, device="cuda") if count else None,
                faces=torch.full((fcap, 3), FACE_POISON, dtype=torch.int32, device="cuda") if faces else None,
                face_count=torch.full((1,), -55, dtype=torch.int32, device="cuda"))


def _gpu_mesh(hip, vol, grid, min_weight=1, capacity=None, face_capacity=None, **which):
    Nx, Ny, Nz = grid["dims"]
    out = _buffers(Nx * Ny * Nz if capacity is None else capacity, 2 * Nx * Ny * Nz if face_capacity is None else face_capacity, **which)
    ws = torch.full((hip.tsdf_mesh_workspace_bytes(Nx, Ny, Nz),), 0xEE, dtype=torch.uint8, device="cuda")
    hip.tsdf_mesh(_dev(vol), **_place(grid), min_weight=min_weight, workspace=ws, **out)
    torch.cuda.synchronize()
    return {k: None if t is None else t.cpu().numpy() for k, t in out.items()}


def _gpu_extract(hip, vol, grid, min_weight, capacity, records=True, gradients=True, count=True):
    Nx, Ny, Nz = grid["dims"]
    out = _buffers(Nx * Ny * Nz if capacity is None else capacity, 0, records, gradients, count)
    del out["faces"], out["face_count"]
    if all(t is None for t in out.values()) or (out["count"] is None and not (Nx * Ny * Nz if capacity is None else capacity)):
        return None                                                         # s2m2_tsdf_extract refuses a call without an output
    ws = torch.full((hip.tsdf_workspace_bytes(Nx, Ny, Nz),), 0xEE, dtype=torch.uint8, device="cuda")
    hip.tsdf_extract(_dev(vol), **_place(grid), min_weight=min_weight, workspace=ws, **out)
    torch.cuda.synchronize()
    return {k: None if t is None else t.cpu().numpy() for k, t in out.items()}


def _check(hip, vol, grid, min_weight=1, capacity=None, face_capacity=None, **which):
    """one K25 call against the oracle and against s2m2_tsdf_extract -> the oracle's dict"""
    m = M.mesh(vol, **_place(grid), min_weight=min_weight)
    got = _gpu_mesh(hip, vol, grid, min_weight, capacity, face_capacity, **which)
    nf, n = m["face_count"], m["count"]
    print(f"[tsdf mesh] dims {grid['dims']} min_weight {min_weight}: {n} vertices, {nf} faces")
    assert int(got["face_count"][0]) == nf
    if got["faces"] is not None:
        k = min(nf, len(got["faces"]))
        bad = np.flatnonzero((got["faces"][:k] != m["faces"][:k]).any(1))
        assert got["faces"][:k].tobytes() == m["faces"][:k].tobytes(), f"{len(bad)} faces differ, first {bad[:3]}: {got['faces'][bad[:3]]} vs {m['faces'][bad[:3]]}"
        assert (got["faces"][k:] == FACE_POISON).all(), "stored beyond min(face_count, face_capacity)"
    if got["count"] is not None:
        assert int(got["count"][0]) == n
    for key, poison in (("records", np.int32(REC_POISON)), ("gradients", F("nan"))):
        if got[key] is None:
            continue
        k = min(n, len(got[key]))
        assert got[key][:k].view(np.int32).tobytes() == m[key][:k].view(np.int32).tobytes()
        assert (got[key][k:].view(np.int32) == np.array(poison).view(np.int32)).all(), "stored beyond min(count, capacity)"
    x = _gpu_extract(hip, vol, grid, min_weight, capacity, **{k: v for k, v in which.items() if k != "faces"})
    if x is not None:
        for key in ("records", "gradients", "count"):
            assert (got[key] is None) == (x[key] is None) and (got[key] is None or got[key].tobytes() == x[key].tobytes()), key
    return m


# ---- 1. dims

@pytest.mark.parametrize("name", ["GRID_A", "GRID_ROW", "GRID_LONG"])
def test_fused_grids(hip, name):
    """awkward dims; Nx = 1 (no cells: no faces, the vertices as extract's); a grid three tiles long whose cells reach into the next tile"""
    grid = getattr(S, name)
    Nx, Ny, Nz = grid["dims"]
    tile = hip.tsdf_tile_voxels(Nx, Ny, Nz)
    m = _check(hip, _fuse(grid, max_weight=2), grid)
    assert m["count"] > 0
    if name == "GRID_ROW":
        assert m["face_count"] == 0
        return
    assert m["face_count"] > 0 and not m["valid"].all()
    if name == "GRID_LONG":
        assert Nx * Ny * Nz == 17871 and Nx * Ny * Nz > 2 * tile and Nx * Ny == 777
        top = m["face_cell"] + Nx * Ny + Nx + 1                          # a cell's last corner
        assert (m["face_cell"] // tile != top // tile).any()


def test_rows_longer_than_a_wave(hip):
    """Nx = 70: rows longer than a wave and no multiple of 64, a tile border inside a slice"""
    grid = _grid((70, 9, 14))
    tile = hip.tsdf_tile_voxels(70, 9, 14)
    assert tile % (70 * 9) and 70 * 9 * 14 > tile
    m = _check(hip, _random_volume(grid["dims"], 21, unobserved=0.03), grid)
    assert m["face_count"] > 1000


# ---- 2. every case

@pytest.mark.parametrize("unobserved", [0.0, 0.1])
def test_all_256_cases(hip, unobserved):
    grid = _grid((20, 19, 18))
    vol = _random_volume(grid["dims"], 7, unobserved)
    case, valid = M.cells(vol)
    assert case.size == 5814 and valid.all() == (unobserved == 0.0) and valid.sum() > 2000
    assert len(np.unique(case[valid])) == 256
    _check(hip, vol, grid)


# ---- 3. exact zeros

def test_exact_zeros_give_coincident_vertices_and_degenerate_triangles(hip):
    grid = dict(dims=(7, 5, 4), origin=(0.0, 0.0, 0.0), voxel_size=0.5)
    g = np.random.default_rng(3)
    vol = O.empty(grid["dims"])
    t = np.where(g.random((4, 5, 7)) < 0.5, 0.5, -0.5).astype(F)
    zero = g.random(t.shape) < 0.3
    t[zero] = np.where(g.random(zero.sum()) < 0.5, 0.0, -0.0).astype(F)
    vol[..., 0], vol[..., 1] = t.view(np.int32), 1
    m = _check(hip, vol, grid)
    bits = t.view(np.int32)
    assert (bits == 0).any() and (bits == np.int32(-2 ** 31)).any()
    p = m["records"][:, :3].view(F)
    tri = p[m["faces"]]
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert (area == 0).any() and (area > 0).any()
    assert len(np.unique(p, axis=0)) < len(p)                           # several vertices on one voxel centre


# ---- 4. min_weight

@pytest.fixture(scope="module")
def fused3():
    """GRID_A after three frames from three poses: weights 0 .. 3"""
    vol = _fuse(S.GRID_A)
    vol.setflags(write=False)
    return vol


@pytest.mark.parametrize("min_weight", [1, 3])
def test_min_weight(hip, fused3, min_weight):
    w = O.unpack(fused3)["weight"]
    assert ((w > 0) & (w < 3)).any() and (w >= 3).any()
    m = _check(hip, fused3, S.GRID_A, min_weight=min_weight)
    other = M.mesh(fused3, **_place(S.GRID_A), min_weight=4 - min_weight)
    assert m["face_count"] > 0 and m["face_count"] != other["face_count"]


# ---- 5. a cell across a tile border

def test_a_cell_straddling_a_tile_border(hip):
    grid = S.GRID_LONG
    Nx, Ny, Nz = grid["dims"]
    tile = hip.tsdf_tile_voxels(Nx, Ny, Nz)
    vol = _random_volume(grid["dims"], 9)
    v = vol.reshape(-1, 4)
    base = tile - 1                                                     # the cell's corners 0 and 1 are the last voxel of a tile and the first of the next
    i, j, k = base % Nx, base // Nx % Ny, base // (Nx * Ny)
    assert i < Nx - 1 and j < Ny - 1 and k < Nz - 1
    for c in range(8):
        v[base + (c & 1) + (c >> 1 & 1) * Nx + (c >> 2) * Nx * Ny, 0] = np.array(-0.5 if c in (0, 3) else 0.25, F).view(np.int32)
    m = _check(hip, vol, grid)
    assert m["case"][k, j, i] == 0b1001 and (m["face_cell"] == base).sum() == 2


# ---- 6. capacities

@pytest.mark.parametrize("case", ["count-only", "face-prefix", "vertex-overflow", "faces-only", "nothing-but-the-count"])
def test_capacities(hip, fused3, case):
    grid = S.GRID_A
    m = M.mesh(fused3, **_place(grid))
    n, nf = m["count"], m["face_count"]
    assert n > 20 and nf > 20
    if case == "count-only":                                            # faces NULL with face_capacity 0
        _check(hip, fused3, grid, faces=False)
    elif case == "face-prefix":                                         # a prefix is stored, the sentinel behind it stays
        _check(hip, fused3, grid, face_capacity=nf - 9)
    elif case == "vertex-overflow":                                     # the faces still carry true ranks
        got = _check(hip, fused3, grid, capacity=n - 7)
        assert got["faces"].max() >= n - 7
    elif case == "faces-only":
        _check(hip, fused3, grid, capacity=0, records=False, gradients=False, count=False)
    else:
        _check(hip, fused3, grid, capacity=0, records=False, gradients=False, count=False, faces=False)


# ---- 7. reproducibility and graph replay

def test_two_runs_and_a_graph_replay_after_a_further_integrate(hip):
    grid = S.GRID_A
    frames = S.frames(["steps", "tilt"], holes=False)
    poses = [np.array([S.IDENTITY, ROT], F), np.array([ROT, S.rot_xy(-0.05, 0.2, (0.0, 0.02, -0.1))], F)]
    expect, vol = [], O.empty(grid["dims"])
    for p in poses:
        vol, _ = O.integrate(vol, *frames, p, **_place(grid), trunc=grid["trunc"], max_weight=64, carve=True, **S.CAM)
        expect.append(M.mesh(vol, **_place(grid)))
    assert expect[0]["face_count"] > 0 and expect[0]["faces"].tobytes() != expect[1]["faces"].tobytes()
    dev = [_dev(a[:, None]) for a in frames[:3]] + [_dev(frames[3])]
    Nx, Ny, Nz = grid["dims"]
    n = Nx * Ny * Nz

    def run(v, pose_buf, out, ws):
        hip.tsdf_integrate(v, *dev, pose_buf, **S.CAM, **_place(grid), trunc=grid["trunc"], max_weight=64, carve=True)
        hip.tsdf_mesh(v, **_place(grid), workspace=ws, **out)

    def fresh():
        return (_dev(O.empty(grid["dims"])), _buffers(n, 2 * n), torch.full((hip.tsdf_mesh_workspace_bytes(Nx, Ny, Nz),), 0xEE, dtype=torch.uint8, device="cuda"),
                _dev(poses[0]))

    def same(out, step):
        torch.cuda.synchronize()
        m = expect[step]
        got = {k: t.cpu().numpy() for k, t in out.items()}
        assert int(got["face_count"][0]) == m["face_count"] and int(got["count"][0]) == m["count"]
        assert got["faces"][:m["face_count"]].tobytes() == m["faces"].tobytes() and got["records"][:m["count"]].tobytes() == m["records"].tobytes()
        assert got["gradients"][:m["count"]].view(np.int32).tobytes() == m["gradients"].view(np.int32).tobytes()
        return [got[k].tobytes() for k in sorted(got)]

    runs = []
    for _ in range(2):                                                  # two eager runs into fresh buffers (also the warm-up of the capture)
        v, out, ws, buf = fresh()
        for step, p in enumerate(poses):
            buf.copy_(_dev(p))
            run(v, buf, out, ws)
            runs.append(same(out, step))
    assert runs[0] == runs[2] and runs[1] == runs[3]                    # bit-identical, the poisoned remainders included
    v, out, ws, buf = fresh()
    graph = torch.cuda.CUDAGraph()                                      # (one stream, no side branches)
    with torch.cuda.graph(graph):
        run(v, buf, out, ws)
    v.zero_()
    for step, p in enumerate(poses):                                    # the pose buffer alone is rewritten between the replays
        buf.copy_(_dev(p))
        graph.replay()
        same(out, step)


# ---- 8. the Python layer

def test_extract_mesh_end_to_end(hip, tmp_path):
    grid = S.GRID_A
    frames = S.frames(KINDS3)
    cam = {k: v for k, v in S.CAM.items() if k != "fy"}
    tv = cloud.TsdfVolume(grid["dims"], grid["voxel_size"], grid["origin"], trunc=grid["trunc"], max_weight=4)
    empty = tv.extract_mesh()
    assert empty.size() == 0 and empty.face_size() == 0                 # an all-zero volume has no surface
    dev = [_dev(a[:, None]) for a in frames[:3]] + [_dev(frames[3])]
    tv.integrate(*dev, R=POSES3.reshape(3, 3, 4)[:, :, :3], t=POSES3.reshape(3, 3, 4)[:, :, 3], **cam)
    m = M.mesh(_fuse(grid, max_weight=4), **_place(grid), min_weight=2)
    mesh = tv.extract_mesh(min_weight=2)
    n, nf = m["count"], m["face_count"]
    Nx, Ny, Nz = grid["dims"]
    assert isinstance(mesh, cloud.TsdfMesh) and mesh.face_capacity() == 2 * Nx * Ny * Nz and mesh.capacity == Nx * Ny * Nz
    assert n > 0 and nf > 0 and mesh.size() == n and mesh.face_size() == nf
    assert mesh.faces().cpu().numpy().tobytes() == m["faces"].tobytes() and mesh.records[0, :n].cpu().numpy().tobytes() == m["records"].tobytes()
    assert mesh.gradients().cpu().numpy().view(np.int32).tobytes() == m["gradients"].view(np.int32).tobytes()
    surf = tv.extract(min_weight=2)                                     # extract's own workspace is untouched by extract_mesh's
    assert surf.records[0, :n].cpu().numpy().tobytes() == m["records"].tobytes()
    assert mesh.write_ply(str(tmp_path / "m.ply")) == (n, nf)
    rec, faces = cloud.read_ply_mesh(str(tmp_path / "m.ply"))
    assert rec.tobytes() == m["records"].tobytes() and faces.tobytes() == m["faces"].tobytes()
    assert mesh.write_ply(str(tmp_path / "n.ply"), normals=True) == (n, nf)
    rec, faces = cloud.read_ply_mesh(str(tmp_path / "n.ply"))
    nrm = mesh.normals().cpu().numpy()
    assert rec.dtype == cloud.NORMAL_RECORD_DTYPE and faces.tobytes() == m["faces"].tobytes()
    assert np.array_equal(rec["x"], m["records"][:, 0].view(F)) and np.array_equal(rec["ny"], nrm[:, 1]) and np.array_equal(rec["red"], m["records"][:, 3] & 0xff)
    small = tv.extract_mesh(min_weight=2, capacity=n, face_capacity=5, want_gradients=False)
    assert small.face_size() == 5 and small.faces().cpu().numpy().tobytes() == m["faces"][:5].tobytes() and small.gradients_buf is None
    with pytest.raises(ValueError, match="unstored vertices"):
        tv.extract_mesh(min_weight=2, capacity=n - 1).faces()


# ---- 9. the runner

def _s_model():
    from s2m2_amd.model import S2M2
    from s2m2_amd.spec import MODEL_CONFIGS
    from s2m2_amd.weights import seeded_state_dict
    C, ntr = MODEL_CONFIGS["S"]
    m = S2M2(C, 1, ntr, use_positivity=True, refine_iter=3)
    m.load_state_dict(seeded_state_dict(C, 1, ntr, 0), strict=True)
    return m.cuda().eval()


def test_runner_meshes_two_frames(hip, tmp_path):
    """s2m2_run_engine --tsdf-frames ... --tsdf-mesh: the mesh PLY equals what TsdfVolume.extract_mesh gives on the maps the same engine writes
    with --out, its vertices are --tsdf-ply's points, and "tsdf_faces" joins the printed line"""
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
            "--depth-trunc", "6", "--conf-min", "0.02", "--tsdf-ply", str(tmp_path / "t.ply")]
    p = subprocess.run(args + ["--tsdf-mesh", str(tmp_path / "m.ply")], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr
    tv = cloud.TsdfVolume(dims, vs, origin, trunc=0.06, max_weight=32767)
    for (maps, image), pose in zip(frames, poses):
        q = np.asarray(pose, np.float64).reshape(3, 4)
        tv.integrate(*maps, image, R=q[:, :3], t=q[:, 3], carve=True, **cam)
    mesh = tv.extract_mesh()
    n, nf = mesh.size(), mesh.face_size()
    print(f"[tsdf mesh runner] {n} vertices, {nf} faces")
    assert n > 0 and nf > 0 and nf <= 4 * n
    assert f'{{"tsdf_frames": 2, "tsdf_points": {n}, "tsdf_faces": {nf}}}' in p.stdout
    rec, faces = cloud.read_ply_mesh(str(tmp_path / "m.ply"))
    assert rec.tobytes() == mesh.records[0, :n].cpu().numpy().tobytes() and faces.tobytes() == mesh.faces().cpu().numpy().tobytes()
    assert cloud.read_ply_records(str(tmp_path / "t.ply")).tobytes() == rec.tobytes()
