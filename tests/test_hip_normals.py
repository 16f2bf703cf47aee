"""K28 on the GPU (include/s2m2_hip.h: s2m2_normals; s2m2_amd/cloud.py: normals, track, write_ply) against the numpy oracle of
tests/normals_oracle.py on the cases of tests/normals_cases.py -- never against the code under test.

What a call owes: depth, normals, image and count as BYTES (the per-pixel rule is fp32 with one rounding per operation, and the count is an
integer sum).  The maps lie in NaN, every output is poisoned before the call with a guard band on either side; the guards, and the outputs
that a call does not request, must still hold the poison.  Frame-to-frame tracking against a normal map is held to what
tests/test_hip_tsdf_track.py holds K27 to: count, status and residual as bytes, each sum within gamma_{n-1} * sum |term| of the exact sum, the
pose within one fp32 spacing plus the oracle's bound."""
import ctypes
import itertools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import normals_cases as C
import normals_oracle as N
import tsdf_scenes as S
import tsdf_track_oracle as T
import tsdf_track_scenes as TS
from s2m2_amd import cloud, utils

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64
ALL = ("depth", "normals", "image", "count")
DTYPE = dict(depth=torch.int32, normals=torch.int32, image=torch.uint8, count=torch.int32)      # the fp32 outputs are poisoned as bit patterns
POISON = dict(depth=0x7fc00123, normals=0x7fc00321, image=0xA5, count=-77)
NAMES = [c["name"] for c in C.cases()]
IDENT = np.array([S.IDENTITY], F)


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


def _bytes(a):
    return np.ascontiguousarray(a).tobytes()


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _binding(kw):
    """the oracle's keywords -> the binding's: filtered becomes unfiltered, depth_trunc None is 0 (no truncation)"""
    kw = dict(kw)
    kw["unfiltered"] = not kw.pop("filtered", True)
    if kw.get("depth_trunc") is None:
        kw["depth_trunc"] = 0.0
    return kw


def _maps(maps, off=0):
    """the maps (B,Hp,Wp) on the device as (B,1,Hp,Wp) views into NaN, `off` floats behind a 16-byte boundary"""
    out = []
    for m in maps:
        flat = torch.full((GUARD + off + m.size + GUARD,), float("nan"), device="cuda")
        flat[GUARD + off:GUARD + off + m.size] = _dev(m.ravel())
        out.append(flat[GUARD + off:GUARD + off + m.size].view(m.shape[0], 1, *m.shape[1:]))
    return out


class Outputs:
    """the four outputs, poisoned, with a guard band on either side; `off` elements (4 bytes of the fp32 outputs and of count, ONE byte of the
    image) behind a 16-byte boundary"""

    def __init__(self, B, H, W, off=0):
        self.shape = dict(depth=(B, 1, H, W), normals=(B, 3, H, W), image=(B, 3, H, W), count=(B,))
        self.n = {k: int(np.prod(s)) for k, s in self.shape.items()}
        self.off = off
        self.flat = {k: torch.full((GUARD + off + self.n[k] + GUARD,), POISON[k], dtype=DTYPE[k], device="cuda") for k in ALL}

    def view(self, k):
        v = self.flat[k][GUARD + self.off:GUARD + self.off + self.n[k]].view(self.shape[k])
        return v.view(torch.float32) if k in ("depth", "normals") else v

    def poisoned(self, k):
        return bool((self.flat[k] == POISON[k]).all())

    def check(self, which):
        """the guards, and the outputs not requested, still hold the poison -> the requested outputs as numpy"""
        torch.cuda.synchronize()
        for k in ALL:
            lo, hi = self.flat[k][:GUARD + self.off], self.flat[k][GUARD + self.off + self.n[k]:]
            assert (lo == POISON[k]).all() and (hi == POISON[k]).all(), f"written outside {k}"
            if k not in which:
                assert self.poisoned(k), f"{k} was not requested"
        return {k: self.view(k).cpu().numpy() for k in which}


def _gpu(hip, c, which=ALL, off=0):
    disp = c["maps"][0]
    out = Outputs(len(disp), c["kw"]["H"], c["kw"]["W"], off)
    hip.normals(*_maps(c["maps"], off), **_binding(c["kw"]), **{k: out.view(k) for k in which})
    return out.check(which)


def _same(got, want, what=""):
    for k, g in got.items():
        e = want[k]
        if k in ("depth", "normals"):
            g, e = g.view(np.int32), e.view(np.int32)
        bad = np.argwhere(g != e)
        assert _bytes(g) == _bytes(e), f"{what} {k}: {len(bad)} differ, first {bad[:3].tolist()}: {[g[tuple(i)] for i in bad[:3]]} vs {[e[tuple(i)] for i in bad[:3]]}"


@pytest.fixture(scope="module")
def oracle():
    return {c["name"]: N.batch(*c["maps"], **c["kw"]) for c in C.cases()}


# ---- 1. every case, as bytes

@pytest.mark.parametrize("name", NAMES)
def test_every_case_as_bytes(hip, oracle, name):
    c = C.by_name(name)
    print(f"[normals] {name}: count {oracle[name]['count'].tolist()}")
    _same(_gpu(hip, c), oracle[name], name)


@pytest.mark.parametrize("name", ["big_padded", "steps_r2", "tilted_cos0.5", "r8_seven_rows", "two_pairs", "spoiled"])
def test_misaligned_bases(hip, oracle, name):
    """maps, depth, normals and count four bytes behind a 16-byte boundary, the image one byte: the per-pixel loads and stores.  The first four
    cases have Wp % 4 == 0 and take the 16-byte map loads when aligned"""
    _same(_gpu(hip, C.by_name(name), off=1), oracle[name], name)


@pytest.mark.parametrize("which", [c for n in range(1, 5) for c in itertools.combinations(ALL, n)], ids="-".join)
def test_every_subset_of_the_outputs(hip, oracle, which):
    _same(_gpu(hip, C.by_name("own_r3"), which), oracle["own_r3"], "own_r3")
    _same(_gpu(hip, C.by_name("steps"), which), oracle["steps"], "steps")


@pytest.mark.parametrize("name", ["big_padded", "spoiled", "spoiled_unfiltered", "two_pairs"])
def test_depth_is_k15s(hip, name):
    c = C.by_name(name)
    kw = _binding(c["kw"])
    B, H, W = len(c["maps"][0]), kw.pop("H"), kw.pop("W")
    got = _gpu(hip, c, ("depth",))["depth"]
    depth = torch.full((B, 1, H, W), -1.0, device="cuda")
    k15 = {k: kw[k] for k in ("fx", "fy", "cx", "cy", "baseline", "doffs", "depth_scale", "depth_trunc", "conf_min", "occ_min", "unfiltered")}
    hip.cloud(*_maps(c["maps"]), torch.zeros((B, 3, H, W), dtype=torch.uint8, device="cuda"), **k15, depth=depth)
    assert _bytes(got.view(np.int32)) == _bytes(depth.cpu().numpy().view(np.int32))


# ---- 2. reproducibility and capture

def test_two_runs_a_graph_replay_and_new_maps_in_place(hip, oracle):
    first = C.by_name("big_padded")
    a, b = _gpu(hip, first), _gpu(hip, first)
    _same(a, b)
    _same(a, oracle["big_padded"])
    maps = _maps(first["maps"])
    out = Outputs(1, first["kw"]["H"], first["kw"]["W"])
    views = {k: out.view(k) for k in ALL}

    def run():
        hip.normals(*maps, **_binding(first["kw"]), **views)

    run()                                                                      # the warm-up of the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()                                             # (one stream, no side branches)
    with torch.cuda.graph(graph):
        run()
    for k in ALL:
        out.flat[k].fill_(POISON[k])
    graph.replay()
    _same(out.check(ALL), oracle["big_padded"], "replay")
    # new maps in place: the frame turned by half a turn, other bytes everywhere (the oracle says what that gives)
    other = [np.ascontiguousarray(m[:, ::-1, ::-1]) for m in first["maps"]]
    want = N.batch(*other, **first["kw"])
    assert _bytes(want["normals"]) != _bytes(oracle["big_padded"]["normals"]) and want["count"][0] > 1000
    for d, m in zip(maps, other):
        d.copy_(_dev(m[:, None]))
    for k in ALL:
        out.flat[k].fill_(POISON[k])
    graph.replay()
    _same(out.check(ALL), want, "replay on new maps")


# ---- 3. errors: non-zero, nothing launched

def _desc(hip, maps, out, kw, which=ALL):
    kw = _binding(kw)
    d = hip.NormalsDesc()
    H, W = kw.pop("H"), kw.pop("W")
    radius, max_jump, min_cos = kw.pop("radius"), kw.pop("max_jump"), kw.pop("min_cos")
    hip._cloud_inputs("normals", d.cloud, *maps, None, H, W, kw["fx"], kw["fy"], kw["cx"], kw["cy"], kw["baseline"], kw["doffs"], kw["depth_scale"],
                      kw["depth_trunc"], kw["conf_min"], kw["occ_min"], kw["unfiltered"])
    for k in which:
        setattr(d, k, out.view(k).data_ptr())
    d.radius, d.max_jump, d.min_cos = radius, max_jump, min_cos
    return d


def _spoil(d, field, value):
    obj = d
    *path, leaf = field.split(".")
    for p in path:
        obj = getattr(obj, p)
    setattr(obj, leaf, value)


ERRORS = [("cloud.disp", None), ("cloud.occ", None), ("cloud.conf", None), ("cloud.disp", "+2"), ("cloud.B", 0), ("cloud.H", 0), ("cloud.W", -1),
          ("cloud.H", 99), ("cloud.W", 141), ("cloud.fx", 0.0), ("cloud.fy", -1.0), ("cloud.depth_scale", 0.0), ("cloud.image_dtype", 7),
          ("depth", "+2"), ("normals", "+2"), ("count", "+1"), ("radius", 0), ("radius", 9), ("radius", -1), ("max_jump", -1e-9),
          ("max_jump", float("nan")), ("max_jump", float("-inf")), ("min_cos", 1.0), ("min_cos", float("nan")), ("min_cos", float("inf")),
          ("min_cos", float("-inf"))]


@pytest.mark.parametrize("field,value", ERRORS, ids=[f"{f}={v}" for f, v in ERRORS])
def test_every_error_launches_nothing(hip, field, value):
    c = C.by_name("big_padded")
    maps = _maps(c["maps"])
    out = Outputs(1, c["kw"]["H"], c["kw"]["W"])
    d = _desc(hip, maps, out, c["kw"])
    if isinstance(value, str):                                                 # the pointer moved by so many bytes
        obj, leaf = (d.cloud, field.split(".")[1]) if "." in field else (d, field)
        setattr(obj, leaf, getattr(obj, leaf) + int(value))
    else:
        _spoil(d, field, value)
    rc = hip.load().s2m2_normals(ctypes.byref(d), hip._stream())
    torch.cuda.synchronize()
    assert rc != 0, f"{field} = {value} was accepted"
    assert all(out.poisoned(k) for k in ALL), "an output was written"


def test_no_descriptor_no_output_and_the_valid_edge(hip, oracle):
    c = C.by_name("big_padded")
    maps = _maps(c["maps"])
    out = Outputs(1, c["kw"]["H"], c["kw"]["W"])
    assert hip.load().s2m2_normals(None, hip._stream()) != 0
    assert hip.load().s2m2_normals(ctypes.byref(_desc(hip, maps, out, c["kw"], ())), hip._stream()) != 0        # no output requested
    torch.cuda.synchronize()
    assert all(out.poisoned(k) for k in ALL)
    with pytest.raises(ValueError, match="no output requested"):
        hip.normals(*maps, **_binding(c["kw"]))
    for bad in (dict(radius=0), dict(radius=9), dict(radius=1.5), dict(max_jump=-1.0), dict(max_jump=float("nan")), dict(min_cos=1.0),
                dict(min_cos=float("nan"))):
        with pytest.raises(ValueError, match=next(iter(bad))):
            hip.normals(*maps, **dict(_binding(c["kw"]), **bad), depth=out.view("depth"))
    assert all(out.poisoned(k) for k in ALL)
    # the descriptor itself is fine: the same one, unspoiled, runs; max_jump = +inf and a min_cos just below 1 are valid
    d = _desc(hip, maps, out, c["kw"])
    assert hip.load().s2m2_normals(ctypes.byref(d), hip._stream()) == 0
    _same(out.check(ALL), oracle["big_padded"])
    d.max_jump, d.min_cos = float("inf"), 1.0 - 2.0 ** -24
    assert hip.load().s2m2_normals(ctypes.byref(d), hip._stream()) == 0
    torch.cuda.synchronize()


# ---- 4. the Python layer: cloud.normals, cloud.track

CAMERA = dict(fx=S.CAM["fx"], cx=S.CAM["cx"], cy=S.CAM["cy"], baseline=S.CAM["baseline"], depth_scale=S.CAM["depth_scale"], depth_trunc=S.CAM["depth_trunc"])
RULE = dict(radius=1, max_jump=1.0, min_cos=0.2)


def _frames(model_pose=tuple(S.IDENTITY), live_pose=tuple(TS.TRUE)):
    (md, mo, mc), mkw = TS.live("own", 51, 73, pose=model_pose)
    (ld, lo, lc), lkw = TS.live("own", 51, 73, pose=live_pose)
    assert mkw == lkw
    return (md, mo, mc), (ld, lo, lc), lkw


def test_cloud_normals_is_a_render(hip, oracle):
    c = C.by_name("own")
    dev = [_dev(m[:, None]) for m in c["maps"]]
    nm = cloud.normals(*dev, H=S.H, W=S.W, **CAMERA, **RULE, want_image=True)
    want = oracle["own"]
    assert isinstance(nm, cloud.TsdfRender) and isinstance(nm, cloud.NormalMap)
    _same(dict(depth=nm.depth.cpu().numpy(), normals=nm.gradients_buf.cpu().numpy(), image=nm.image.cpu().numpy(), count=nm.count.cpu().numpy()), want)
    assert _bytes(nm.poses.cpu().numpy()) == _bytes(IDENT) and tuple(nm.R.shape) == (1, 3, 3)
    cam = nm.camera
    assert (cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy) == (S.W, S.H, S.CAM["fx"], S.CAM["fx"], S.CAM["cx"], S.CAM["cy"])
    assert nm.holes() == S.H * S.W - int(want["count"][0])
    assert np.abs(nm.normals().cpu().numpy() - want["normals"]).max() < 1e-6
    bare = cloud.normals(*dev, H=S.H, W=S.W, **CAMERA, **RULE, want_count=False)
    assert bare.image is None and bare.count is None and _bytes(bare.gradients_buf.cpu().numpy()) == _bytes(want["normals"])
    # the maps' own size is the default crop: the padded frame as a whole
    whole = cloud.normals(*dev, **dict(CAMERA, cx=S.CAM["cx"] + 3, cy=S.CAM["cy"] + 3), **RULE)
    e = N.batch(*c["maps"], **dict(c["kw"], H=51, W=73, cx=S.CAM["cx"] + 3, cy=S.CAM["cy"] + 3))
    assert _bytes(whole.gradients_buf.cpu().numpy()) == _bytes(e["normals"])


def test_cloud_track_against_a_normal_map(hip):
    """one iteration against K27's oracle on the ORACLE's normals, as test_hip_tsdf_track.py's _check1 holds K27; then ten iterations under the
    condition of the CPU test"""
    model, live, kw = _frames()
    on = N.normals(*model, **kw, **RULE)
    args = dict(kw, **TS.model_kw(), **TS.GATES)
    o = T.iterate(*live, IDENT[0], IDENT[0], on["depth"], on["normals"], **args)
    assert o["status"] == 0 and o["count"] > 1000
    nm = cloud.normals(*[_dev(m[None, None]) for m in model], H=S.H, W=S.W, **CAMERA, **RULE)
    dev = [_dev(m[None, None]) for m in live]
    gates = dict(max_dist=TS.GATES["max_dist"], min_count=TS.GATES["min_count"], max_rot=TS.GATES["max_rot"], max_trans=TS.GATES["max_trans"])
    tr = cloud.track(*dev, nm, H=S.H, W=S.W, **CAMERA, **gates, n_iters=1, want_residual=True)
    row, pose = tr.systems.cpu().numpy()[0, 0], tr.poses.cpu().numpy()[0]
    print(f"[normals track] count {o['count']} (gpu {row[28]:.0f}) status {o['status']} (gpu {row[29]:.0f}) kappa {o['kappa']:.3g} bound {o['bound']:.3g}")
    assert _bytes(row[28:30]) == _bytes(o["row"][28:30]), "count / status"
    assert _bytes(tr.residual.cpu().numpy()[0, 0].view(np.int32)) == _bytes(o["residual"].view(np.int32)), "residual"
    n = o["count"]
    err, lim = T.sum_errors(o["J"], o["r"], row[:28]), T.gamma(n - 1) * o["abs"]
    print(f"[normals track]   sums: largest error / bound {np.max(err / np.maximum(lim, 1e-300)):.3g}")
    assert (err <= lim).all(), (err, lim)
    tol = np.spacing(np.abs(o["P"]).astype(F)).astype(np.float64) + o["bound"]
    d = np.abs(pose.astype(np.float64) - o["P"])
    print(f"[normals track]   pose: largest error / tolerance {np.max(d / tol):.3g}")
    assert (d <= tol).all(), (pose, o["P"])
    assert tr.ok() and tr.count() == n
    # ten iterations from the identity (the default start), both errors to a fifth at the most: of the oracle first
    ten = T.track(*[m[None] for m in live], IDENT, IDENT, on["depth"][None, None], on["normals"][None], n_iters=10, **args)
    r0, t0 = T.pose_errors(S.IDENTITY, TS.TRUE)
    ro, to = T.pose_errors(ten["poses"][0], TS.TRUE)
    assert ro <= r0 / 5 and to <= t0 / 5
    tr = cloud.track(*dev, nm, H=S.H, W=S.W, **CAMERA, **gates, n_iters=10)
    r1, t1 = T.pose_errors(tr.poses.cpu().numpy()[0], TS.TRUE)
    print(f"[normals track] rotation {r0:.3g} -> {r1:.3g} (oracle {ro:.3g}), translation {t0:.3g} -> {t1:.3g} (oracle {to:.3g})")
    assert r1 <= r0 / 5 and t1 <= t0 / 5 and (tr.systems.cpu().numpy()[0, :, 29] == 0).all()
    # R and t, a pose buffer refined in place, and the checks of the start
    buf = _dev(IDENT)
    tr2 = cloud.track(*dev, nm, poses=buf, H=S.H, W=S.W, **CAMERA, **gates, n_iters=10, want_systems=False)
    assert tr2.poses is buf and tr2.systems is None and _bytes(buf.cpu().numpy()) == _bytes(tr.poses.cpu().numpy())
    tr3 = cloud.track(*dev, nm, R=np.eye(3), t=np.zeros(3), H=S.H, W=S.W, **CAMERA, **gates, n_iters=10)
    assert _bytes(tr3.poses.cpu().numpy()) == _bytes(tr.poses.cpu().numpy())
    with pytest.raises(ValueError, match="either"):
        cloud.track(*dev, nm, poses=buf, R=np.eye(3), t=np.zeros(3), H=S.H, W=S.W, **CAMERA, **gates)
    with pytest.raises(TypeError):
        cloud.track(*dev, nm, H=S.H, W=S.W, **CAMERA)                           # max_dist and max_trans have no default


def test_normals_then_track_captured_once(hip):
    """no volume and no ray-cast: normals -> track captured once, then replayed on a second pair of frames (the first pair the other way
    round); a replay gives what the eager calls give on the same frames, byte for byte"""
    model, live, kw = _frames()
    gates = dict(max_dist=TS.GATES["max_dist"], min_count=TS.GATES["min_count"], max_rot=TS.GATES["max_rot"], max_trans=TS.GATES["max_trans"])
    dm, dl = [_dev(m[None, None]) for m in model], [_dev(m[None, None]) for m in live]
    pbuf = _dev(IDENT)
    keep = {}

    def run(m, l, p):
        nm = cloud.normals(*m, H=S.H, W=S.W, **CAMERA, **RULE, want_count=False)
        return cloud.track(*l, nm, poses=p, H=S.H, W=S.W, **CAMERA, **gates, n_iters=6)

    run(dm, dl, pbuf)                                                          # the warm-up of the capture (and of track's workspace)
    torch.cuda.synchronize()
    pbuf.copy_(_dev(IDENT))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep["tr"] = run(dm, dl, pbuf)
    for pair in ((model, live), (live, model)):
        eager = run([_dev(m[None, None]) for m in pair[0]], [_dev(m[None, None]) for m in pair[1]], _dev(IDENT))
        for d, m in zip(dm + dl, pair[0] + pair[1]):
            d.copy_(_dev(m[None, None]))
        pbuf.copy_(_dev(IDENT))
        graph.replay()
        torch.cuda.synchronize()
        assert _bytes(pbuf.cpu().numpy()) == _bytes(eager.poses.cpu().numpy()) and _bytes(pbuf.cpu().numpy()) != _bytes(IDENT)
        assert _bytes(keep["tr"].systems.cpu().numpy()) == _bytes(eager.systems.cpu().numpy())
        assert (eager.systems.cpu().numpy()[0, :, 29] == 0).all()
    # the second pair is the first the other way round: the motions are inverse to each other, as far as six iterations get
    P = pbuf.cpu().numpy()[0].astype(np.float64).reshape(3, 4)
    inv = np.concatenate([P[:, :3].T, (-P[:, :3].T @ P[:, 3])[:, None]], 1).ravel()
    r0, t0 = T.pose_errors(S.IDENTITY, TS.TRUE)
    r1, t1 = T.pose_errors(inv, TS.TRUE)
    assert r1 <= r0 / 5 and t1 <= t0 / 5


# ---- 5. PLY files with normals

def _read_ply_normals(path):
    raw = open(path, "rb").read()
    end = raw.find(b"end_header\n") + len(b"end_header\n")
    n = int([line for line in raw[:end].decode("ascii").split("\n") if line.startswith("element vertex")][0].split()[2])
    assert raw[:end].decode("ascii") == cloud.PLY_NORMALS_HEADER % n and len(raw) == end + n * cloud.NORMAL_RECORD_DTYPE.itemsize
    return np.frombuffer(raw[end:], dtype=cloud.NORMAL_RECORD_DTYPE)


@pytest.mark.parametrize("name", ["spoiled", "two_pairs"])
def test_ply_files_with_normals(hip, oracle, tmp_path, name):
    c = C.by_name(name)
    dev = [_dev(m[:, None]) for m in c["maps"]]
    B = len(c["maps"][0])
    image = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (B, 3, S.H, S.W)).astype(np.uint8)).cuda()
    nm = cloud.normals(*dev, H=S.H, W=S.W, **CAMERA, **RULE)
    pc = cloud.reproject(*dev, image, **CAMERA)
    ms = cloud.mesh(*dev, image, **CAMERA)
    want = oracle[name]
    for b in range(B):
        kept = want["depth"][b, 0] > 0
        n = int(kept.sum())
        assert n == pc.size(b) and 0 < want["count"][b] <= n
        assert name != "spoiled" or want["count"][b] < n                       # some kept pixels have no normal: they get 0,0,0
        rec = pc.records[b, :n].cpu().numpy().view(cloud.RECORD_DTYPE).ravel()
        wn = want["normals"][b][:, kept].T
        # the cloud
        path = str(tmp_path / f"cloud{b}.ply")
        assert pc.write_ply(path, b, normals=nm) == n
        got = _read_ply_normals(path)
        for f in cloud.RECORD_DTYPE.names:
            assert _bytes(got[f]) == _bytes(rec[f]), f
        assert _bytes(np.stack([got["nx"], got["ny"], got["nz"]], 1)) == _bytes(wn)
        # the mesh
        path = str(tmp_path / f"mesh{b}.ply")
        assert ms.write_ply(path, b, normals=nm) == (n, ms.face_size(b))
        verts, faces = cloud.read_ply_mesh(path)
        assert verts.dtype == cloud.NORMAL_RECORD_DTYPE and _bytes(verts) == _bytes(got) and _bytes(faces) == _bytes(ms.faces(b).cpu().numpy())
        # without normals: the bytes of the plain writers
        plain, ref = str(tmp_path / f"plain{b}.ply"), str(tmp_path / f"ref{b}.ply")
        pc.write_ply(plain, b)
        cloud.write_ply_records(ref, pc.records[b, :n].cpu().numpy())
        assert open(plain, "rb").read() == open(ref, "rb").read()
        ms.write_ply(plain, b, normals=None)
        cloud.write_ply_mesh(ref, ms.records[b, :n].cpu().numpy(), ms.faces(b).cpu().numpy())
        assert open(plain, "rb").read() == open(ref, "rb").read()
    # another filter keeps other pixels; a capacity below the count has no record for every normal
    other = cloud.normals(*dev, H=S.H, W=S.W, **dict(CAMERA, depth_trunc=2.0), **RULE)
    with pytest.raises(ValueError, match="not the same maps"):
        pc.write_ply(str(tmp_path / "x.ply"), 0, normals=other)
    short = cloud.reproject(*dev, image, **CAMERA, capacity=10)
    with pytest.raises(ValueError, match="capacity"):
        short.write_ply(str(tmp_path / "x.ply"), 0, normals=nm)


def test_utils_get_normals(hip):
    """get_pointcloud's conventions: halved intrinsics, fx for both focal lengths, the disparity as all three maps, no filter"""
    calib = dict(cam0=np.array([[128.0, 0, 67.0], [0, 120.0, 45.0], [0, 0, 1]]), baseline=15.625, doffs=0.0, width=2 * S.W, height=2 * S.H)
    (disp, _, _), kw = TS.live(Hp=S.H, Wp=S.W, pose=tuple(S.IDENTITY))
    nm = utils.get_normals(disp, calib, depth_trunc=10.0, radius=2, max_jump=0.5, min_cos=0.1)
    args = dict(kw, baseline=15.625, depth_scale=1000.0, filtered=False)       # baseline * fx = 15.625 * 64 = 1000: the scene's z = 1 / d
    e = N.normals(disp, disp, disp, **args, radius=2, max_jump=0.5, min_cos=0.1)
    assert e["count"] > 1000 and int(nm.count[0].item()) == e["count"]
    assert _bytes(nm.depth.cpu().numpy()[0, 0]) == _bytes(e["depth"]) and _bytes(nm.gradients_buf.cpu().numpy()[0]) == _bytes(e["normals"])


# ---- 6. the runner

def _s_model():
    from s2m2_amd.model import S2M2
    from s2m2_amd.spec import MODEL_CONFIGS
    from s2m2_amd.weights import seeded_state_dict
    C_, ntr = MODEL_CONFIGS["S"]
    m = S2M2(C_, 1, ntr, use_positivity=True, refine_iter=3)
    m.load_state_dict(seeded_state_dict(C_, 1, ntr, 0), strict=True)
    return m.cuda().eval()


def test_runner_writes_the_normal_map(hip, tmp_path):
    """s2m2_run_engine --normals --normals-image --normals-radius 2: a plumbing test -- the files equal what cloud.normals gives on the maps the
    same run writes with --out, as bytes, and the JSON line parses"""
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
    left, right = synthetic_pair(H, W, 1, 24, 11)
    names = [str(tmp_path / n) for n in ("left.f32", "right.f32")]
    for name, t in zip(names, (left, right)):
        open(name, "wb").write(t.contiguous().numpy().astype("<f4").tobytes())
    out = tmp_path / "out"
    out.mkdir()
    args = [RUNNER, engine, *names, "--out", str(out), "--calib", calib_path, "--depth-trunc", "6", "--conf-min", "0.02", "--max-jump", "0.5",
            "--normals", str(tmp_path / "n.f32"), "--normals-image", str(tmp_path / "n.ppm"), "--normals-radius", "2", "--normals-min-cos", "0.1",
            "--repeat", "2"]
    p = subprocess.run(args, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr
    maps = [torch.from_numpy(np.fromfile(out / f"{n}.f32", dtype="<f4").reshape(1, 1, H, W)).cuda() for n in ("disp", "occ", "conf")]
    nm = cloud.normals(*maps, **cam, radius=2, max_jump=0.5, min_cos=0.1, want_image=True)
    n = int(nm.count[0].item())
    print(f"[normals runner] {n} of {H * W} pixels have a normal")
    assert open(tmp_path / "n.f32", "rb").read() == _bytes(nm.gradients_buf.cpu().numpy())
    ppm = open(tmp_path / "n.ppm", "rb").read()
    head = f"P6\n{W} {H}\n255\n".encode("ascii")
    assert ppm[:len(head)] == head and ppm[len(head):] == _bytes(nm.image[0].permute(1, 2, 0).contiguous().cpu().numpy())
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('{"normals_count"')]
    assert len(line) == 1
    js = json.loads(line[0])
    assert set(js) == {"normals_count", "repeat", "normals_us_per_pair"} and js["normals_count"] == n and js["repeat"] == 2
    assert js["normals_us_per_pair"] > 0
    # the rules between the options
    for bad, msg in ((["--normals", "x.f32"], "--normals needs --calib"), (["--calib", calib_path, "--normals-radius", "2"], "need --normals"),
                     (["--calib", calib_path, "--normals", "x.f32", "--normals-radius", "9"], "--normals-radius"),
                     (["--calib", calib_path, "--normals", "x.f32", "--normals-min-cos", "1"], "--normals-min-cos")):
        q = subprocess.run([RUNNER, engine, *names, *bad], capture_output=True, text=True, timeout=60)
        assert q.returncode != 0 and msg in q.stderr, (bad, q.stderr)
