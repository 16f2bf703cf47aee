"""K15 on the GPU (include/s2m2_hip.h: s2m2_cloud; s2m2_amd/cloud.py): validity filter, depth and the compacted point cloud against the numpy
oracle of tests/cloud_oracle.py -- never against the code under test.  Every pixel of every case takes part in every comparison: the synthetic
maps are drawn so that no value lies within 1e-6 of a threshold, and the oracle evaluates the same fp32 chain.

z and the dense depth are compared BIT FOR BIT (the library is built with -fno-fast-math: fp32 division is correctly rounded, and the chain has
no multiply-add pair that contraction could fuse).  x, y are compared with the float64 oracle under
    |err| <= 4 * 2^-23 * |x| + 2^-23 * |cx| * z / fx        (y: cy, fy)
-- the conversion of cx to fp32 gives the absolute term (it dominates near the principal point), three fp32 roundings (subtraction, product,
quotient) the relative one with a margin of two.  Record order is checked position by position against the oracle's raster-order kept list,
through the pixel index recovered from each record."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import cloud_oracle
from s2m2_amd import cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(ROOT, "tests", "golden", "bicycle2_calib.txt")
EPS = 2.0 ** -23
PATTERN = 0x5A5A5A5A


def _calib():
    c = cloud.read_calib_file(CALIB)
    return dict(fx=float(c["cam0"][0, 0]), fy=float(c["cam0"][1, 1]), cx=float(c["cam0"][0, 2]), cy=float(c["cam0"][1, 2]),
                baseline=float(c["baseline"]), doffs=float(c["doffs"]))


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


@functools.lru_cache(maxsize=2)
def _maps(Hp, Wp, B, seed):
    """disp uniform in [-20, 300], conf / occ uniform in [0, 1]; values within 1e-3 px / 1e-6 of a decision threshold are moved away from it"""
    g = np.random.default_rng(seed)
    k = _calib()
    disp = (g.random((B, 1, Hp, Wp), dtype=np.float32) * np.float32(320.0) - np.float32(20.0)).astype(np.float32)
    conf = g.random((B, 1, Hp, Wp), dtype=np.float32)
    occ = g.random((B, 1, Hp, Wp), dtype=np.float32)
    t_trunc = k["baseline"] * k["fx"] / (3.0 * 1000.0) - k["doffs"]                  # z = 3 m at this disparity (61.5 px)
    disp[(np.abs(disp) < 1e-3) | (np.abs(disp - t_trunc) < 1e-3)] = 100.0
    conf[np.abs(conf - 0.1) < 1e-6] = 0.2
    occ[np.abs(occ - 0.5) < 1e-6] = 0.6
    return disp, occ, conf


@functools.lru_cache(maxsize=2)
def _image(B, H, W, dtype_name, seed):
    g = np.random.default_rng(seed + 17)
    u8 = g.integers(0, 256, (B, 3, H, W), dtype=np.uint8)
    if dtype_name == "uint8":
        return u8
    # float images: fractions (ties k + 0.5 among them, both parities of k) and values beyond both ends of [0, 255]
    frac = g.choice(np.array([0.0, 0.25, 0.5, 0.75], dtype=np.float32), size=u8.shape)
    f = u8.astype(np.float32) + frac
    f[g.random(u8.shape) < 0.01] = -3.5
    f[g.random(u8.shape) < 0.01] = 260.0
    return f.astype(np.float16 if dtype_name == "float16" else np.float32)


@functools.lru_cache(maxsize=1)
def _oracle(Hp, Wp, H, W, B, seed, filtered, trunc):
    disp, occ, conf = _maps(Hp, Wp, B, seed)
    dummy = np.zeros((3, H, W), dtype=np.uint8)
    return [cloud_oracle.cloud(cloud_oracle.crop(disp[b, 0], H, W), cloud_oracle.crop(occ[b, 0], H, W), cloud_oracle.crop(conf[b, 0], H, W), dummy,
                               depth_trunc=trunc, filtered=filtered, **_calib()) for b in range(B)]


def _check_pair(o, rgb_all, rec, n, k, H, W, depth=None, mask=None, stored=None):
    """one pair against its oracle `o` (cloud_oracle.cloud): rec = the stored records as a RECORD_DTYPE array, n = the device count"""
    index = o["index"]
    assert n == len(index), (n, len(index))
    m = len(index) if stored is None else stored
    assert len(rec) == m
    if mask is not None:
        assert np.array_equal(mask.astype(bool), o["keep"])
    if depth is not None:
        assert np.array_equal(depth.view(np.int32), o["depth"].view(np.int32))
    if m == 0:
        return
    z = rec["z"]
    assert np.array_equal(z.view(np.int32), o["z"][:m].view(np.int32)), "z differs from the fp32 chain of the oracle"
    # raster order: the pixel every record came from, position by position
    z64 = z.astype(np.float64)
    u = np.rint(rec["x"].astype(np.float64) * k["fx"] / z64 + k["cx"]).astype(np.int64)
    v = np.rint(rec["y"].astype(np.float64) * k["fy"] / z64 + k["cy"]).astype(np.int64)
    assert np.array_equal(v * W + u, index[:m])
    ex = np.abs(rec["x"].astype(np.float64) - o["x64"][:m])
    ey = np.abs(rec["y"].astype(np.float64) - o["y64"][:m])
    bx = 4 * EPS * np.abs(o["x64"][:m]) + EPS * abs(k["cx"]) * z64 / k["fx"]
    by = 4 * EPS * np.abs(o["y64"][:m]) + EPS * abs(k["cy"]) * z64 / k["fy"]
    assert (ex <= bx).all(), float((ex / bx).max())
    assert (ey <= by).all(), float((ey / by).max())
    want = rgb_all.reshape(3, H * W)[:, index[:m]].T
    got = np.stack([rec["red"], rec["green"], rec["blue"]], axis=1)
    assert np.array_equal(got, want)
    assert (rec["alpha"] == 255).all()


def _records(pc, b, stored):
    return pc.records[b, :stored].cpu().numpy().view(cloud.RECORD_DTYPE).reshape(-1)


# The last three are shapes of tests/test_hip_mesh.py, whose vertex launch is K15's scatter kernel: map width no multiple of 4 (the per-pixel
# kernels) with crop offset 1; the aligned kernels with ox % 4 == 1 over three tiles of 67 rows; five block steps per row (both buffers of the
# rank step are reused), one row per tile
SIZES = [(1024, 1216, 1024, 1216), (1024, 1216, 1000, 1190), (32, 32, 1, 1), (2048, 2432, 2000, 2400),
         (40, 63, 37, 61), (160, 64, 140, 61), (32, 4128, 3, 4100)]
CASES = [(s, B, f, t, dt) for s in SIZES for B in (1, 3) for f in (True, False) for t in (3.0, None) for dt in ("uint8", "float16", "float32")]


@pytest.mark.parametrize("size,B,filtered,trunc,dtype_name", CASES,
                         ids=[f"{s[1]}x{s[0]}-{s[3]}x{s[2]}-b{B}-{'filt' if f else 'all'}-trunc{t}-{dt}" for s, B, f, t, dt in CASES])
def test_operator_against_the_oracle(hip, size, B, filtered, trunc, dtype_name):
    Hp, Wp, H, W = size
    seed = Hp * 7 + W + B
    k = _calib()
    disp, occ, conf = (torch.from_numpy(a).cuda() for a in _maps(Hp, Wp, B, seed))
    img = _image(B, H, W, dtype_name, seed)
    pc = cloud.reproject(disp, occ, conf, torch.from_numpy(img).cuda(), depth_trunc=trunc, filtered=filtered, want_depth=True, want_mask=True, **k)
    torch.cuda.synchronize()
    oracle = _oracle(Hp, Wp, H, W, B, seed, filtered, trunc)
    counts = pc.count.cpu().numpy()
    depth, mask = pc.depth.cpu().numpy(), pc.mask.cpu().numpy()
    kept = 0
    for b in range(B):
        n = int(counts[b])
        kept += n
        _check_pair(oracle[b], cloud_oracle.colour_bytes(img[b]), _records(pc, b, min(n, H * W)), n, k, H, W, depth[b, 0], mask[b, 0])
        assert pc.points(b).shape == (n, 3) and pc.colors(b).shape == (n, 3)
    if trunc is None:
        assert kept == B * H * W                     # without truncation the 1e9 sentinel is a point too, as in the reference
    elif H * W > 1000:
        share = kept / (B * H * W)
        assert (0.30 < share < 0.37) if filtered else (0.72 < share < 0.78), share


def _const_maps(B, Hp, Wp, disp, conf, occ):
    f = lambda v: torch.full((B, 1, Hp, Wp), v, device="cuda", dtype=torch.float32)
    return f(disp), f(occ), f(conf)


def test_every_pixel_kept(hip):
    Hp, Wp, H, W = 1024, 1216, 1000, 1190
    k = _calib()
    disp, occ, conf = _const_maps(1, Hp, Wp, 100.0, 1.0, 1.0)
    img = _image(1, H, W, "uint8", 5)
    pc = cloud.reproject(disp, occ, conf, torch.from_numpy(img).cuda(), **k)
    torch.cuda.synchronize()
    assert int(pc.count[0]) == H * W
    rec = _records(pc, 0, H * W)
    z = np.float32(np.float32(k["baseline"] * k["fx"]) / (np.float32(100.0) + np.float32(k["doffs"]))) / np.float32(1000.0)
    assert (rec["z"] == z).all()
    for r, (v, u) in ((rec[0], (0, 0)), (rec[-1], (H - 1, W - 1))):
        assert r["x"] == (np.float32(u) - np.float32(k["cx"])) * z / np.float32(k["fx"])
        assert r["y"] == (np.float32(v) - np.float32(k["cy"])) * z / np.float32(k["fy"])
        assert (r["red"], r["green"], r["blue"], r["alpha"]) == (img[0, 0, v, u], img[0, 1, v, u], img[0, 2, v, u], 255)
    o = cloud_oracle.cloud(np.full((H, W), 100.0, np.float32), np.ones((H, W), np.float32), np.ones((H, W), np.float32), img[0], **k)
    _check_pair(o, img[0], rec, H * W, k, H, W)


def _direct(hip, maps, img, k, records, trunc=3.0, filtered=True):
    B, _, H, W = img.shape
    count = torch.full((B,), -7, device="cuda", dtype=torch.int32)
    ws = torch.empty(hip.cloud_workspace_bytes(B, H, W), device="cuda", dtype=torch.uint8)
    hip.cloud(*maps, img, depth_trunc=trunc, unfiltered=not filtered, records=records, count=count, workspace=ws, **k)
    torch.cuda.synchronize()
    return count


def test_no_pixel_kept_leaves_the_records_untouched(hip):
    Hp, Wp, H, W = 1024, 1216, 1000, 1190
    maps = _const_maps(1, Hp, Wp, 100.0, 0.0, 1.0)               # confidence 0 everywhere: d = -1 -> the sentinel, beyond 3 m
    img = torch.from_numpy(_image(1, H, W, "uint8", 6)).cuda()
    records = torch.full((1, H * W, 4), PATTERN, device="cuda", dtype=torch.int32)
    count = _direct(hip, maps, img, _calib(), records)
    assert int(count[0]) == 0
    assert bool((records == PATTERN).all())


def test_capacity_below_the_count(hip):
    """count stays the true number, the first `capacity` records are right, and a guard region right behind the buffer keeps its pattern (read
    back: the absence of an out-of-bounds store is observed in memory, nothing is provoked)"""
    Hp, Wp, H, W = 1024, 1216, 1000, 1190
    B, seed, k = 1, 99, _calib()
    maps = tuple(torch.from_numpy(a).cuda() for a in _maps(Hp, Wp, B, seed))
    imgn = _image(B, H, W, "uint8", seed)
    o = _oracle(Hp, Wp, H, W, B, seed, True, 3.0)[0]
    true = len(o["index"])
    cap, guard = true // 2, 4096
    assert cap > 1000
    buf = torch.full((1, cap + guard, 4), PATTERN, device="cuda", dtype=torch.int32)
    count = _direct(hip, maps, torch.from_numpy(imgn).cuda(), k, buf[:, :cap])
    assert int(count[0]) == true
    assert bool((buf[:, cap:] == PATTERN).all())
    rec = buf[0, :cap].cpu().numpy().view(cloud.RECORD_DTYPE).reshape(-1)
    _check_pair(o, imgn[0], rec, true, k, H, W, stored=cap)
    # capacity 0: the count alone
    count = _direct(hip, maps, torch.from_numpy(imgn).cuda(), k, torch.empty((1, 0, 4), device="cuda", dtype=torch.int32))
    assert int(count[0]) == true


def test_two_runs_are_byte_identical_also_on_poisoned_lds(hip):
    Hp, Wp, H, W = 1024, 1216, 1000, 1190
    B, seed, k = 3, 41, _calib()
    maps = tuple(torch.from_numpy(a).cuda() for a in _maps(Hp, Wp, B, seed))
    img = torch.from_numpy(_image(B, H, W, "float16", seed)).cuda()
    first = cloud.reproject(*maps, img, depth_trunc=3.0, **k)
    torch.cuda.synchronize()
    hip.poison_lds()
    second = cloud.reproject(*maps, img, depth_trunc=3.0, **k)
    torch.cuda.synchronize()
    assert torch.equal(first.count, second.count)
    for b in range(B):
        n = first.size(b)
        assert n > 0 and torch.equal(first.records[b, :n], second.records[b, :n])


def test_hipgraph_capture_and_replay_after_the_maps_change(hip):
    Hp, Wp, H, W = 1024, 1216, 1000, 1190
    B, k = 1, _calib()
    draws = [_maps(Hp, Wp, B, s) for s in (201, 202)]
    draws = [tuple(a.copy() for a in d) for d in draws]
    imgn = _image(B, H, W, "uint8", 201)
    img = torch.from_numpy(imgn).cuda()
    maps = tuple(torch.from_numpy(a).cuda() for a in draws[0])
    records = torch.zeros((B, H * W, 4), device="cuda", dtype=torch.int32)
    count = torch.zeros((B,), device="cuda", dtype=torch.int32)
    depth = torch.zeros((B, 1, H, W), device="cuda", dtype=torch.float32)
    ws = torch.empty(hip.cloud_workspace_bytes(B, H, W), device="cuda", dtype=torch.uint8)
    kw = dict(depth_trunc=3.0, records=records, count=count, workspace=ws, depth=depth, **k)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.cloud(*maps, img, **kw)                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hip.cloud(*maps, img, **kw)
    for d in draws:
        for t, a in zip(maps, d):
            t.copy_(torch.from_numpy(a))                         # in place: the graph keeps reading the same buffers
        records.fill_(PATTERN)
        count.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        o = cloud_oracle.cloud(*(cloud_oracle.crop(a[0, 0], H, W) for a in d), imgn[0], depth_trunc=3.0, **k)
        n = int(count[0])
        rec = records[0, :n].cpu().numpy().view(cloud.RECORD_DTYPE).reshape(-1)
        _check_pair(o, imgn[0], rec, n, k, H, W, depth=depth[0, 0].cpu().numpy())
    assert len(o["index"]) != 0


# ------------------------------------------------------------------------------------------------ end to end

def _s_model():
    from s2m2_amd.model import S2M2
    from s2m2_amd.spec import MODEL_CONFIGS
    from s2m2_amd.weights import seeded_state_dict
    C, ntr = MODEL_CONFIGS["S"]
    m = S2M2(C, 1, ntr, use_positivity=True, refine_iter=3)
    m.load_state_dict(seeded_state_dict(C, 1, ntr, 0), strict=True)
    return m.cuda().eval()


@pytest.mark.parametrize("H,W", [(384, 512), (375, 500)])
def test_forward_then_reproject(hip, H, W):
    from s2m2_amd import utils
    from s2m2_amd.weights import synthetic_pair
    m = _s_model()
    left, right = synthetic_pair(H, W, 1, 24, 3)
    left_u8, right_u8 = left.to(torch.uint8).cuda(), right.to(torch.uint8).cuda()
    lp, rp = utils.image_pad(left_u8, 32), utils.image_pad(right_u8, 32)
    with torch.autocast("cuda", dtype=torch.float16):
        maps = [t.float().contiguous() for t in m(lp, rp)]
    torch.cuda.synchronize()
    disp, occ, conf = maps
    assert disp.shape[-2:] == (-(-H // 32) * 32, -(-W // 32) * 32)
    k = _calib()
    imgn = left_u8.cpu().numpy()
    host = [utils.image_crop(t.cpu(), (H, W))[0, 0].numpy() for t in (disp, occ, conf)]
    for filtered, trunc in ((True, 3.0), (False, 3.0), (False, None)):
        pc = cloud.reproject(disp, occ, conf, left_u8, depth_trunc=trunc, filtered=filtered, want_depth=True, want_mask=True, **k)
        torch.cuda.synchronize()
        o = cloud_oracle.cloud(*host, imgn[0], depth_trunc=trunc, filtered=filtered, **k)
        n = int(pc.count[0])
        print(f"[cloud e2e] {W}x{H} filtered={filtered} trunc={trunc}: {n} of {H * W} pixels kept")
        _check_pair(o, imgn[0], _records(pc, 0, n), n, k, H, W, pc.depth[0, 0].cpu().numpy(), pc.mask[0, 0].cpu().numpy())
    assert n == H * W
    # utils.get_pointcloud (the reference's argument list, halved intrinsics, no filter of its own) on the cropped, filtered disparity
    calib = cloud.read_calib_file(CALIB)
    valid = (host[2] > np.float32(0.1)) & (host[1] > np.float32(0.5))
    dfilt = np.where(valid, host[0], np.float32(-1.0)).astype(np.float32)
    rgb = np.ascontiguousarray(imgn[0].transpose(1, 2, 0))
    half = dict(k, fx=k["fx"] / 2.0, fy=k["fx"] / 2.0, cx=k["cx"] / 2.0, cy=k["cy"] / 2.0)
    for trunc in (None, 1.9):
        a = utils.get_pointcloud(rgb, dfilt, calib, depth_trunc=trunc)
        b = cloud.reproject(disp, occ, conf, left_u8, depth_trunc=trunc, filtered=True, **half)
        torch.cuda.synchronize()
        na = int(a.count[0])
        print(f"[cloud e2e] get_pointcloud trunc={trunc}: {na} points")
        assert na == int(b.count[0]) and (na == H * W if trunc is None else na <= H * W)
        assert torch.equal(a.records[0, :na], b.records[0, :na])
        assert tuple(a.points().shape) == (na, 3) and a.colors().dtype == torch.uint8


def test_runner_writes_the_cloud(hip, tmp_path):
    from s2m2_amd.build import RUNNER
    from s2m2_amd.export import export_engine
    from s2m2_amd.weights import synthetic_pair
    H, W = 384, 512
    m = _s_model()
    path = str(tmp_path / "s_384x512.s2m2")
    export_engine(m, path, H, W)
    left, right = synthetic_pair(H, W, 1, 24, 11)
    left, right = left.contiguous(), right.contiguous()
    (tmp_path / "left.f32").write_bytes(left.numpy().astype("<f4").tobytes())
    (tmp_path / "right.f32").write_bytes(right.numpy().astype("<f4").tobytes())
    left_u8 = left.to(torch.uint8)
    (tmp_path / "left.u8").write_bytes(left_u8.numpy().tobytes())
    base = [RUNNER, path, str(tmp_path / "left.f32"), str(tmp_path / "right.f32")]
    k = _calib()

    def run(tag, extra):
        out = tmp_path / tag
        out.mkdir()
        p = subprocess.run(base + ["--out", str(out)] + extra, capture_output=True, text=True, timeout=240)
        assert p.returncode == 0, p.stderr
        return out, p.stdout

    def maps_of(out):
        return [torch.from_numpy(np.fromfile(out / f"{n}.f32", dtype="<f4").reshape(1, 1, H, W)).cuda() for n in ("disp", "occ", "conf")]

    # the issue's invocation: colours from the engine's own float32 left input
    a, _ = run("a", ["--calib", CALIB, "--depth-trunc", "3", "--ply", str(tmp_path / "a.ply"), "--depth", str(tmp_path / "a_depth.f32")])
    pc = cloud.reproject(*maps_of(a), left.cuda(), depth_trunc=3.0, want_depth=True, **k)
    torch.cuda.synchronize()
    rec = cloud.read_ply_records(str(tmp_path / "a.ply"))
    n = int(pc.count[0])
    print(f"[cloud runner] --depth-trunc 3: {n} vertices")
    assert len(rec) == n and rec.tobytes() == pc.records[0, :n].cpu().numpy().tobytes()
    assert (tmp_path / "a_depth.f32").read_bytes() == pc.depth.cpu().numpy().tobytes()
    # every pixel (no filter, no truncation), colours from a uint8 file, and the timing line of --repeat
    b, stdout = run("b", ["--calib", CALIB, "--unfiltered", "--image", str(tmp_path / "left.u8"), "--ply", str(tmp_path / "b.ply"), "--repeat", "3"])
    assert "ms_per_pair" in stdout and "cloud_us_per_pair" in stdout
    pc = cloud.reproject(*maps_of(b), left_u8.cuda(), filtered=False, **k)
    torch.cuda.synchronize()
    rec = cloud.read_ply_records(str(tmp_path / "b.ply"))
    assert len(rec) == H * W == int(pc.count[0]) and rec.tobytes() == pc.records[0].cpu().numpy().tobytes()
    ply = tmp_path / "tmp.ply"
    assert pc.write_ply(str(ply)) == H * W and ply.read_bytes() == (tmp_path / "b.ply").read_bytes()
    # without the new options: the same maps, byte for byte, and nothing else written
    c, stdout = run("c", [])
    assert stdout == ""
    for name in ("disp.f32", "occ.f32", "conf.f32"):
        assert (c / name).read_bytes() == (a / name).read_bytes() == (b / name).read_bytes()
    assert sorted(os.listdir(c)) == ["conf.f32", "disp.f32", "occ.f32"]
    # option errors are usage errors, before the engine is loaded
    p = subprocess.run(base + ["--ply", str(tmp_path / "x.ply")], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--calib and --ply come together" in p.stderr
