"""K29 on the GPU (include/s2m2_hip.h: s2m2_smooth, s2m2_smooth_weights; s2m2_amd/cloud.py: smooth) against the numpy oracle of
tests/smooth_oracle.py on the cases of tests/smooth_cases.py -- never against the code under test.  The oracle is fed the LIBRARY's weight
tables (s2m2_smooth_weights), which are themselves held to one fp32 ulp of the oracle's.

What a call owes: disp_out (the whole padded map, border included), taps and count as BYTES (the per-pixel rule is fp32 with one rounding per
operation and a fixed order of additions, and the count is an integer sum).  The maps lie in NaN, every output is poisoned before the call
with a guard band on either side; the guards, and the outputs that a call does not request, must still hold the poison."""
import ctypes
import itertools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import normals_oracle as N
import smooth_cases as C
import smooth_oracle as O
import tsdf_scenes as S
import tsdf_track_oracle as T
import tsdf_track_scenes as TS
from s2m2_amd import cloud, utils

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64
ALL = ("disp_out", "taps", "count")
POISON = dict(disp_out=0x7fc00123, taps=-55, count=-77)      # the fp32 output is poisoned as a bit pattern
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


def _binding(c):
    """the case's keywords -> the binding's: filtered becomes unfiltered, depth_trunc None is 0 (no truncation), the two widths"""
    kw = dict(c["kw"], sigma_s=c["sigma"][0], sigma_r=c["sigma"][1])
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
    """the three outputs, poisoned, with a guard band on either side; `off` elements of four bytes behind a 16-byte boundary"""

    def __init__(self, B, Hp, Wp, H, W, off=0):
        self.shape = dict(disp_out=(B, 1, Hp, Wp), taps=(B, 1, H, W), count=(B,))
        self.n = {k: int(np.prod(s)) for k, s in self.shape.items()}
        self.off = off
        self.flat = {k: torch.full((GUARD + off + self.n[k] + GUARD,), POISON[k], dtype=torch.int32, device="cuda") for k in ALL}

    def view(self, k):
        v = self.flat[k][GUARD + self.off:GUARD + self.off + self.n[k]].view(self.shape[k])
        return v.view(torch.float32) if k == "disp_out" else v

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


def _outputs(c, off=0):
    B, Hp, Wp = c["maps"][0].shape
    return Outputs(B, Hp, Wp, c["kw"]["H"], c["kw"]["W"], off)


def _gpu(hip, c, which=ALL, off=0):
    out = _outputs(c, off)
    hip.smooth(*_maps(c["maps"], off), **_binding(c), **{k: out.view(k) for k in which})
    return out.check(which)


def _same(got, want, what=""):
    for k, g in got.items():
        e = want[k]
        if k == "disp_out":
            g, e = g.view(np.int32), e.view(np.int32)
        bad = np.argwhere(g != e)
        assert _bytes(g) == _bytes(e), f"{what} {k}: {len(bad)} differ, first {bad[:3].tolist()}: {[g[tuple(i)] for i in bad[:3]]} vs {[e[tuple(i)] for i in bad[:3]]}"


@pytest.fixture(scope="module")
def oracle(hip):
    """smooth_oracle on every case, with the tables the library itself uses"""
    return {c["name"]: C.oracle(c, hip.smooth_weights) for c in C.cases()}


# ---- 1. the tables

def test_the_librarys_tables_are_the_oracles_within_one_ulp(hip):
    differ = total = 0
    for r, ss, sr in [(c["kw"]["radius"], *c["sigma"]) for c in C.cases()] + [(8, 4.0, 0.06), (1, 0.3, 1e-3), (5, 100.0, 50.0), (8, 0.05, 2.0)]:
        ws, wr, inv = hip.smooth_weights(r, ss, sr)
        es, er, ei = O.tables(r, ss, sr)
        assert ws.dtype == F and wr.dtype == F and ws.shape == (9,) and wr.shape == (257,)
        assert ws[0] == 1 and wr[0] == 1 and not ws[r + 1:].any()
        for got, want in ((ws, es), (wr, er), (np.array([inv], F), np.array([ei], F))):
            assert (np.abs(got.astype(np.float64) - want) <= np.spacing(want)).all(), (r, ss, sr)
            differ += int((got != want).sum())
            total += got.size
    print(f"[smooth] tables: {differ} of {total} entries differ from numpy's (each by one ulp)")
    for bad in ((0, 1.0, 1.0), (9, 1.0, 1.0), (2, 0.0, 1.0), (2, 1.0, -1.0), (2, float("nan"), 1.0), (2, 1.0, float("inf"))):
        ws, wr, inv = np.zeros(9, F), np.zeros(257, F), ctypes.c_float(0)
        fp = ctypes.POINTER(ctypes.c_float)
        assert hip.load().s2m2_smooth_weights(int(bad[0]), bad[1], bad[2], ws.ctypes.data_as(fp), wr.ctypes.data_as(fp), ctypes.byref(inv)) != 0, bad
    assert hip.load().s2m2_smooth_weights(2, 1.0, 1.0, None, None, None) != 0


# ---- 2. every case, as bytes

@pytest.mark.parametrize("name", NAMES)
def test_every_case_as_bytes(hip, oracle, name):
    print(f"[smooth] {name}: count {oracle[name]['count'].tolist()}, taps up to {oracle[name]['taps'].max()}")
    _same(_gpu(hip, C.by_name(name)), oracle[name], name)


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("name", ["big_padded_r8", "big_unpadded_r5", "steps_r5", "two_pairs", "spoiled", "edge"])
def test_misaligned_bases(hip, oracle, name, off):
    """maps and outputs 4, 8 and 12 bytes behind a 16-byte boundary: the per-pixel loads and stores"""
    _same(_gpu(hip, C.by_name(name), off=off), oracle[name], name)


@pytest.mark.parametrize("which", [c for n in range(1, 4) for c in itertools.combinations(ALL, n)], ids="-".join)
def test_every_subset_of_the_outputs(hip, oracle, which):
    _same(_gpu(hip, C.by_name("own_r3"), which), oracle["own_r3"], "own_r3")
    _same(_gpu(hip, C.by_name("steps_r2"), which), oracle["steps_r2"], "steps_r2")


# ---- 3. reproducibility and capture

def test_two_runs_give_equal_bytes(hip, oracle):
    for name in ("big_padded_r8", "edge"):
        a, b = _gpu(hip, C.by_name(name)), _gpu(hip, C.by_name(name))
        _same(a, b)
        _same(a, oracle[name])


CAMERA = dict(fx=S.CAM["fx"], cx=S.CAM["cx"], cy=S.CAM["cy"], baseline=S.CAM["baseline"], depth_scale=S.CAM["depth_scale"], depth_trunc=S.CAM["depth_trunc"])
RULE = dict(radius=2, sigma_s=1.0, sigma_r=0.03, max_jump=0.25)
NRULE = dict(radius=1, max_jump=1.0, min_cos=0.2)


def test_smooth_normals_track_captured_once_and_replayed_on_new_maps(hip):
    """smooth -> normals(filtered=False) -> track (one iteration) captured once, replayed on two pairs of frames written in place (the
    second is the first the other way round).  Each replay equals the chain of the three oracles: the smoothed map and the normal map as
    bytes, the count and status of the tracking step as bytes and its sums within K27's bound gamma_{n-1} * sum |term|"""
    (md, mo, mc), kw = TS.live("own", 51, 73, pose=tuple(S.IDENTITY))
    (ld, lo, lc), lkw = TS.live("own", 51, 73, pose=tuple(TS.TRUE))
    assert kw == lkw
    gates = dict(max_dist=TS.GATES["max_dist"], min_count=TS.GATES["min_count"], max_rot=TS.GATES["max_rot"], max_trans=TS.GATES["max_trans"])
    dm, dl = [_dev(m[None, None]) for m in (md, mo, mc)], [_dev(m[None, None]) for m in (ld, lo, lc)]
    pbuf = _dev(IDENT)
    keep = {}

    def run():
        s = cloud.smooth(*dm, H=S.H, W=S.W, **CAMERA, **RULE, want_taps=True)
        nm = cloud.normals(s.disp, dm[1], dm[2], H=S.H, W=S.W, **CAMERA, **NRULE, filtered=False)
        return s, nm, cloud.track(*dl, nm, poses=pbuf, H=S.H, W=S.W, **CAMERA, **gates, n_iters=1)

    run()                                                                      # the warm-up of the capture (and of track's workspace)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep["s"], keep["nm"], keep["tr"] = run()
    ws, wr, inv = hip.smooth_weights(RULE["radius"], RULE["sigma_s"], RULE["sigma_r"])
    for model, live in (((md, mo, mc), (ld, lo, lc)), ((ld, lo, lc), (md, mo, mc))):
        for d, m in zip(dm + dl, model + live):
            d.copy_(_dev(m[None, None]))
        pbuf.copy_(_dev(IDENT))
        graph.replay()
        torch.cuda.synchronize()
        so = O.smooth(*model, **kw, radius=RULE["radius"], max_jump=RULE["max_jump"], ws=ws, wr=wr, inv=inv)
        assert so["count"] > 1000
        assert _bytes(keep["s"].disp.cpu().numpy()[0, 0]) == _bytes(so["disp_out"]) and _bytes(keep["s"].taps.cpu().numpy()[0, 0]) == _bytes(so["taps"])
        assert keep["s"].kept() == so["count"]
        on = N.normals(so["disp_out"], model[1], model[2], **dict(kw, filtered=False), **NRULE)
        assert on["count"] > 1000
        assert _bytes(keep["nm"].depth.cpu().numpy()[0, 0]) == _bytes(on["depth"])
        assert _bytes(keep["nm"].gradients_buf.cpu().numpy()[0]) == _bytes(on["normals"])
        o = T.iterate(*live, IDENT[0], IDENT[0], on["depth"], on["normals"], **dict(kw, **TS.model_kw(), **TS.GATES))
        row = keep["tr"].systems.cpu().numpy()[0, 0]
        assert o["status"] == 0 and o["count"] > 1000
        assert _bytes(row[28:30]) == _bytes(o["row"][28:30]), "count / status"
        err, lim = T.sum_errors(o["J"], o["r"], row[:28]), T.gamma(o["count"] - 1) * o["abs"]
        print(f"[smooth chain] kept {so['count']}, normals {on['count']}, correspondences {o['count']}, sums: largest error / bound "
              f"{np.max(err / np.maximum(lim, 1e-300)):.3g}")
        assert (err <= lim).all(), (err, lim)
        tol = np.spacing(np.abs(o["P"]).astype(F)).astype(np.float64) + o["bound"]
        assert (np.abs(pbuf.cpu().numpy()[0].astype(np.float64) - o["P"]) <= tol).all()


# ---- 4. errors: non-zero, nothing launched

def _desc(hip, maps, out, c, which=ALL):
    kw = _binding(c)
    d = hip.SmoothDesc()
    hip._cloud_inputs("smooth", d.cloud, *maps, None, kw["H"], kw["W"], kw["fx"], kw["fy"], kw["cx"], kw["cy"], kw["baseline"], kw["doffs"],
                      kw["depth_scale"], kw["depth_trunc"], kw["conf_min"], kw["occ_min"], kw["unfiltered"])
    for k in which:
        setattr(d, k, out.view(k).data_ptr())
    d.radius, d.sigma_s, d.sigma_r, d.max_jump = kw["radius"], kw["sigma_s"], kw["sigma_r"], kw["max_jump"]
    return d


ERRORS = [("cloud.disp", None), ("cloud.occ", None), ("cloud.conf", None), ("cloud.disp", "+2"), ("cloud.occ", "+1"), ("cloud.B", 0), ("cloud.H", 0),
          ("cloud.W", -1), ("cloud.H", 99), ("cloud.W", 141), ("cloud.fx", 0.0), ("cloud.fy", -1.0), ("cloud.depth_scale", 0.0),
          ("cloud.image_dtype", 7), ("disp_out", "+2"), ("taps", "+2"), ("count", "+1"), ("radius", 0), ("radius", 9), ("radius", -1),
          ("sigma_s", 0.0), ("sigma_s", -1.0), ("sigma_s", float("nan")), ("sigma_s", float("inf")), ("sigma_r", 0.0), ("sigma_r", -0.5),
          ("sigma_r", float("nan")), ("sigma_r", float("inf")), ("max_jump", -1e-9), ("max_jump", float("nan")), ("max_jump", float("-inf"))]


@pytest.mark.parametrize("field,value", ERRORS, ids=[f"{f}={v}" for f, v in ERRORS])
def test_every_error_launches_nothing(hip, field, value):
    c = C.by_name("big_padded_r2")
    maps = _maps(c["maps"])
    out = _outputs(c)
    d = _desc(hip, maps, out, c)
    obj, leaf = (d.cloud, field.split(".")[1]) if "." in field else (d, field)
    setattr(obj, leaf, getattr(obj, leaf) + int(value) if isinstance(value, str) else value)       # a string: the pointer moved by so many bytes
    rc = hip.load().s2m2_smooth(ctypes.byref(d), hip._stream())
    torch.cuda.synchronize()
    assert rc != 0, f"{field} = {value} was accepted"
    assert all(out.poisoned(k) for k in ALL), "an output was written"


def test_no_descriptor_no_output_in_place_and_the_valid_edge(hip, oracle):
    c = C.by_name("big_padded_r2")
    maps = _maps(c["maps"])
    out = _outputs(c)
    assert hip.load().s2m2_smooth(None, hip._stream()) != 0
    assert hip.load().s2m2_smooth(ctypes.byref(_desc(hip, maps, out, c, ())), hip._stream()) != 0              # no output requested
    d = _desc(hip, maps, out, c)
    d.disp_out = d.cloud.disp                                                                                # in place: blocks read each other's halo
    assert hip.load().s2m2_smooth(ctypes.byref(d), hip._stream()) != 0
    torch.cuda.synchronize()
    assert all(out.poisoned(k) for k in ALL) and _bytes(maps[0].cpu().numpy()[:, 0]) == _bytes(c["maps"][0])
    with pytest.raises(ValueError, match="no output requested"):
        hip.smooth(*maps, **_binding(c))
    for bad in (dict(radius=0), dict(radius=9), dict(radius=1.5), dict(max_jump=-1.0), dict(max_jump=float("nan")), dict(sigma_s=0.0),
                dict(sigma_r=float("inf")), dict(sigma_r=float("nan"))):
        with pytest.raises(ValueError, match=next(iter(bad))):
            hip.smooth(*maps, **dict(_binding(c), **bad), count=out.view("count"))
    assert all(out.poisoned(k) for k in ALL)
    # the descriptor itself is fine: the same one, unspoiled, runs; max_jump = +inf and 0 are valid
    d = _desc(hip, maps, out, c)
    assert hip.load().s2m2_smooth(ctypes.byref(d), hip._stream()) == 0
    _same(out.check(ALL), oracle["big_padded_r2"])
    for mj in (float("inf"), 0.0):
        d.max_jump = mj
        assert hip.load().s2m2_smooth(ctypes.byref(d), hip._stream()) == 0
    torch.cuda.synchronize()


# ---- 5. the Python layer

@pytest.mark.parametrize("name", ["spoiled", "two_pairs"])
def test_cloud_smooth_feeds_reproject(hip, oracle, name):
    """Smoothed.disp into reproject(..., filtered=False): exactly the oracle's kept pixels, at the z of their smoothed disparities"""
    c = C.by_name(name)
    want = oracle[name]
    dev = [_dev(m[:, None]) for m in c["maps"]]
    B = len(c["maps"][0])
    r, (ss, sr) = c["kw"]["radius"], c["sigma"]
    s = cloud.smooth(*dev, H=S.H, W=S.W, **CAMERA, radius=r, sigma_r=sr, max_jump=c["kw"]["max_jump"], want_taps=True)      # sigma_s None: radius / 2
    assert isinstance(s, cloud.Smoothed) and ss == r / 2.0
    _same(dict(disp_out=s.disp.cpu().numpy(), taps=s.taps.cpu().numpy(), count=s.count.cpu().numpy()), want, name)
    bare = cloud.smooth(*dev, H=S.H, W=S.W, **CAMERA, radius=r, sigma_s=ss, sigma_r=sr, max_jump=c["kw"]["max_jump"], want_count=False)
    assert bare.taps is None and bare.count is None and _bytes(bare.disp.cpu().numpy()) == _bytes(want["disp_out"])
    with pytest.raises(ValueError, match="want_count"):
        bare.kept()
    with pytest.raises(TypeError):
        cloud.smooth(*dev, H=S.H, W=S.W, **CAMERA)                              # sigma_r and max_jump have no default
    image = torch.zeros((B, 3, S.H, S.W), dtype=torch.uint8, device="cuda")
    pc = cloud.reproject(s.disp, dev[1], dev[2], image, **CAMERA, filtered=False, want_depth=True)
    depth = pc.depth.cpu().numpy()
    for b in range(B):
        kept = want["cls"][b] != O.NOT_KEPT
        assert s.kept(b) == kept.sum() == pc.size(b) and _bytes(depth[b, 0] > 0) == _bytes(kept)
        d = want["disp_out"][b, 0, 3:3 + S.H, 3:3 + S.W]
        z = (F(S.CAM["baseline"] * S.CAM["fx"]) / (d + F(0.0))) / F(S.CAM["depth_scale"])
        assert _bytes(depth[b, 0][kept]) == _bytes(z[kept])


def test_utils_smooth_disparity(hip):
    """get_normals's conventions: halved intrinsics, fx for both focal lengths, the disparity as all three maps, no filter"""
    calib = dict(cam0=np.array([[128.0, 0, 67.0], [0, 120.0, 45.0], [0, 0, 1]]), baseline=15.625, doffs=0.0, width=2 * S.W, height=2 * S.H)
    (disp, _, _), kw = TS.live(Hp=S.H, Wp=S.W, pose=tuple(S.IDENTITY))
    s = utils.smooth_disparity(disp, calib, 0.03, 0.25, depth_trunc=10.0, radius=3)
    ws, wr, inv = hip.smooth_weights(3, 1.5, 0.03)
    e = O.smooth(disp, disp, disp, **dict(kw, baseline=15.625, depth_scale=1000.0, filtered=False), radius=3, max_jump=0.25, ws=ws, wr=wr, inv=inv)
    assert e["count"] > 1000 and s.kept() == e["count"] and _bytes(s.disp.cpu().numpy()[0, 0]) == _bytes(e["disp_out"])


# ---- 6. the runner

def _s_model():
    from s2m2_amd.model import S2M2
    from s2m2_amd.spec import MODEL_CONFIGS
    from s2m2_amd.weights import seeded_state_dict
    C_, ntr = MODEL_CONFIGS["S"]
    m = S2M2(C_, 1, ntr, use_positivity=True, refine_iter=3)
    m.load_state_dict(seeded_state_dict(C_, 1, ntr, 0), strict=True)
    return m.cuda().eval()


def test_runner_smooths_in_front_of_the_normals(hip, tmp_path):
    """s2m2_run_engine --smooth 2 ... --smooth-out --normals: the smoothed map is the oracle's on the maps the same run writes with --out, as
    bytes; the normal map behind it is normals_oracle's on the smoothed map; the JSON line parses; --smooth without its parameters is refused"""
    from s2m2_amd.build import RUNNER
    from s2m2_amd.export import export_engine
    from s2m2_amd.weights import synthetic_pair
    H, W = 384, 512
    calib_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bicycle2_calib.txt")
    k = cloud.read_calib_file(calib_path)
    cam = dict(fx=float(k["cam0"][0, 0]), fy=float(k["cam0"][1, 1]), cx=float(k["cam0"][0, 2]), cy=float(k["cam0"][1, 2]),
               baseline=float(k["baseline"]), doffs=float(k["doffs"]), depth_trunc=6.0, conf_min=0.02)
    engine = str(tmp_path / "s_384x512.s2m2")
    export_engine(_s_model(), engine, H, W)
    left, right = synthetic_pair(H, W, 1, 24, 11)
    names = [str(tmp_path / n) for n in ("left.f32", "right.f32")]
    for name, t in zip(names, (left, right)):
        open(name, "wb").write(t.contiguous().numpy().astype("<f4").tobytes())
    out = tmp_path / "out"
    out.mkdir()
    args = [RUNNER, engine, *names, "--out", str(out), "--calib", calib_path, "--depth-trunc", "6", "--conf-min", "0.02", "--max-jump", "0.5",
            "--smooth", "2", "--smooth-sigma-r", "0.5", "--smooth-max-jump", "1.5", "--smooth-sigma-s", "1.25", "--smooth-out", str(tmp_path / "s.f32"),
            "--normals", str(tmp_path / "n.f32"), "--normals-radius", "2", "--normals-min-cos", "0.1", "--repeat", "2"]
    p = subprocess.run(args, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr
    maps = [np.fromfile(out / f"{n}.f32", dtype="<f4").reshape(H, W) for n in ("disp", "occ", "conf")]
    ws, wr, inv = hip.smooth_weights(2, 1.25, 0.5)
    so = O.smooth(*maps, H=H, W=W, **cam, depth_scale=1000.0, radius=2, max_jump=1.5, ws=ws, wr=wr, inv=inv)
    print(f"[smooth runner] {so['count']} of {H * W} pixels kept, taps up to {so['taps'].max()}")
    assert so["count"] > 1000 and open(tmp_path / "s.f32", "rb").read() == _bytes(so["disp_out"])
    on = N.normals(so["disp_out"], maps[1], maps[2], H=H, W=W, **cam, depth_scale=1000.0, filtered=False, radius=2, max_jump=0.5, min_cos=0.1)
    assert on["count"] > 1000 and open(tmp_path / "n.f32", "rb").read() == _bytes(on["normals"])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('{"smooth_kept"')]
    assert len(line) == 1
    js = json.loads(line[0])
    assert set(js) == {"smooth_kept", "repeat", "smooth_us_per_pair"} and js["smooth_kept"] == so["count"] and js["repeat"] == 2
    assert js["smooth_us_per_pair"] > 0
    # the rules between the options
    full = ["--calib", calib_path, "--smooth", "2", "--smooth-sigma-r", "0.5", "--smooth-max-jump", "1.5"]
    for bad, msg in ((["--calib", calib_path, "--smooth", "2"], "--smooth needs --smooth-sigma-r and --smooth-max-jump"),
                     (["--calib", calib_path, "--smooth", "2", "--smooth-sigma-r", "0.5"], "--smooth needs --smooth-sigma-r and --smooth-max-jump"),
                     (["--calib", calib_path, "--smooth-sigma-r", "0.5"], "need --smooth"), (full[2:], "--smooth needs --calib"),
                     (full[:3] + ["9"] + full[4:], "--smooth: the radius"), (full + ["--smooth-sigma-s", "0"], "--smooth-sigma-s"),
                     (full[:-1] + ["-1"], "--smooth-max-jump")):
        q = subprocess.run([RUNNER, engine, *names, *bad], capture_output=True, text=True, timeout=60)
        assert q.returncode != 0 and msg in q.stderr, (bad, q.stderr)
