"""K21 on the GPU (include/s2m2_hip.h: s2m2_register; s2m2_amd/cloud.py: register): the z-buffered forward warp against the numpy oracle of
tests/register_oracle.py -- never against the code under test -- and against expectations built without any arithmetic (the identity target,
the right view of an integer-disparity scene, everything on one pixel, nothing at all).

Every comparison is EXACT and leaves no pixel out: depth_t as int32 bits, index_t, image_t, visible and count with array_equal.  The oracle
evaluates the same fp32 chain, one rounding per operation, the library is built with -fno-fast-math (correctly rounded division) and the
kernel's chain is compiled with contraction off, so there is no threshold for a value to sit near; the z-buffer is a minimum of unique keys,
which does not depend on the order of arrival."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import cloud_oracle
import register_oracle
from s2m2_amd import cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(ROOT, "tests", "golden", "bicycle2_calib.txt")
F = np.float32
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


@functools.lru_cache(maxsize=4)
def _maps(Hp, Wp, B, seed, odd=True):
    """the draw of tests/test_hip_cloud.py -- disp uniform in [-20, 300], conf / occ uniform in [0, 1], values within 1e-3 px / 1e-6 of a
    decision threshold moved away from it -- plus (odd) a handful of NaN / +inf / -inf disparities per pair, spread over the whole map"""
    g = np.random.default_rng(seed)
    k = _calib()
    disp = (g.random((B, 1, Hp, Wp), dtype=F) * F(320.0) - F(20.0)).astype(F)
    conf = g.random((B, 1, Hp, Wp), dtype=F)
    occ = g.random((B, 1, Hp, Wp), dtype=F)
    t_trunc = k["baseline"] * k["fx"] / (3.0 * 1000.0) - k["doffs"]                  # z = 3 m at this disparity (61.5 px)
    disp[(np.abs(disp) < 1e-3) | (np.abs(disp - t_trunc) < 1e-3)] = 100.0
    conf[np.abs(conf - 0.1) < 1e-6] = 0.2
    occ[np.abs(occ - 0.5) < 1e-6] = 0.6
    if odd:
        for b in range(B):
            flat = disp[b, 0].reshape(-1)
            where = g.choice(flat.size, size=12, replace=False)
            flat[where] = np.tile(np.array([np.nan, np.inf, -np.inf], dtype=F), 4)
    return disp, occ, conf


@functools.lru_cache(maxsize=4)
def _image(B, H, W, dtype_name, seed):
    g = np.random.default_rng(seed + 17)
    u8 = g.integers(0, 256, (B, 3, H, W), dtype=np.uint8)
    if dtype_name == "uint8":
        return u8
    # float images: fractions (ties k + 0.5 among them, both parities of k) and values beyond both ends of [0, 255]
    frac = g.choice(np.array([0.0, 0.25, 0.5, 0.75], dtype=F), size=u8.shape)
    f = u8.astype(F) + frac
    f[g.random(u8.shape) < 0.01] = -3.5
    f[g.random(u8.shape) < 0.01] = 260.0
    return f.astype(np.float16 if dtype_name == "float16" else F)


def _rotation(ax_deg, ay_deg, az_deg):
    ax, ay, az = (math.radians(a) for a in (ax_deg, ay_deg, az_deg))
    rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]])
    return rz @ ry @ rx


def _target(kind, H, W):
    """identity: cam0 itself at the source's size.  rot: a camera of another size (48x80, or 768x1024 behind the large shape) and focal length,
    rotated by 3 / -2 / 1.5 degrees about x / y / z and moved by (0.05, -0.02, 0.03) m, its principal point placed so that the source's centre
    pixel at 2 m lands on the target's centre.  half: cam0 with the principal point moved left by half a width and up by a third of a height:
    half of the projected scene lies outside the target, and the target's right and lower parts stay empty."""
    k = _calib()
    if kind == "identity":
        return cloud.Camera(W, H, k["fx"], k["fy"], k["cx"], k["cy"])
    if kind == "half":
        return cloud.Camera(W, H, k["fx"], k["fy"], k["cx"] - W / 2.0, k["cy"] - H / 3.0)
    assert kind == "rot"
    Ht, Wt = (768, 1024) if H * W > 100000 else (48, 80)
    R, t = _rotation(3.0, -2.0, 1.5), np.array([0.05, -0.02, 0.03])
    fx_t = k["fx"] * Wt / W * 0.9
    fy_t = k["fy"] * Ht / H * 0.85
    p = R @ (np.array([((W - 1) / 2.0 - k["cx"]) / k["fx"], ((H - 1) / 2.0 - k["cy"]) / k["fy"], 1.0]) * 2.0) + t
    return cloud.Camera(Wt, Ht, fx_t, fy_t, Wt / 2.0 - fx_t * p[0] / p[2], Ht / 2.0 - fy_t * p[1] / p[2], R, t)


def _oracle(maps, img, H, W, cam, splat, **kw):
    """one oracle result per pair; maps: the padded (B,1,Hp,Wp) numpy maps, img: (B,3,H,W) numpy or None"""
    disp, occ, conf = maps
    return [register_oracle.register(cloud_oracle.crop(disp[b, 0], H, W), cloud_oracle.crop(occ[b, 0], H, W), cloud_oracle.crop(conf[b, 0], H, W),
                                     None if img is None else img[b], Ht=cam.height, Wt=cam.width, fx_t=cam.fx, fy_t=cam.fy, cx_t=cam.cx,
                                     cy_t=cam.cy, R=cam.R, t=cam.t, splat=splat, **kw) for b in range(disp.shape[0])]


def _check(reg, oracle, tag=""):
    """a Registered against the per-pair oracle results: every output, every pixel, exactly"""
    depth, index = reg.depth.cpu().numpy(), reg.index.cpu().numpy()
    for b, o in enumerate(oracle):
        assert np.array_equal(index[b, 0], o["index_t"]), f"{tag}: index_t of pair {b}: {int((index[b, 0] != o['index_t']).sum())} pixels differ"
        assert np.array_equal(depth[b, 0].view(np.int32), o["depth_t"].view(np.int32)), f"{tag}: depth_t bits of pair {b}"
        if reg.image is not None:
            assert np.array_equal(reg.image[b].cpu().numpy(), o["image_t"]), f"{tag}: image_t of pair {b}"
        if reg.visible is not None:
            assert np.array_equal(reg.visible[b, 0].cpu().numpy(), o["visible"]), f"{tag}: visible of pair {b}"
        if reg.count is not None:
            n = int(reg.count[b].item())
            assert n == o["count"] == int((index[b, 0] >= 0).sum()), f"{tag}: count of pair {b}"


SMALL = [(40, 63, 37, 61), (160, 64, 140, 61), (32, 4128, 3, 4100)]     # the per-pixel kernels with crop offset 1; the aligned kernels with
LARGE = (1024, 1216, 1000, 1190)                                        # ox % 4 == 1 over several tiles; five block steps per row; the flagship


def _cases():
    """every shape x target x splat 1, 2, 3, splat 4 on the first small shape; B, the image dtype and the filter rotate through the cases of
    the small shapes so that each value meets each target and each splat; the large shape runs uint8, with one case of three pairs"""
    out, i = [], 0
    dtypes = ("uint8", "float16", "float32")
    for s in SMALL:
        for kind in ("identity", "rot", "half"):
            for splat in ((1, 2, 3, 4) if s == SMALL[0] else (1, 2, 3)):
                out.append((s, kind, splat, (1, 3)[i % 2], dtypes[(i // 2) % 3], (i // 3) % 2 == 0))
                i += 1
    for kind in ("identity", "rot", "half"):
        for splat in (1, 2, 3):
            out.append((LARGE, kind, splat, 3 if (kind, splat) == ("rot", 2) else 1, "uint8", (kind, splat) != ("half", 3)))
    return out


CASES = _cases()


def test_the_case_list_covers_every_parameter():
    small = [c for c in CASES if c[0] != LARGE]
    assert {c[3] for c in small} == {1, 3} and {c[4] for c in small} == {"uint8", "float16", "float32"} and {c[5] for c in small} == {True, False}
    assert {c[2] for c in small} == {1, 2, 3, 4} and {c[2] for c in CASES if c[0] == LARGE} == {1, 2, 3}
    for kind in ("identity", "rot", "half"):
        here = [c for c in small if c[1] == kind]
        assert {c[3] for c in here} == {1, 3} and {c[5] for c in here} == {True, False} and len({c[4] for c in here}) == 3


@pytest.mark.parametrize("size,kind,splat,B,dtype_name,filtered", CASES,
                         ids=[f"{s[1]}x{s[0]}-{s[3]}x{s[2]}-{kind}-splat{sp}-b{B}-{dt}-{'filt' if f else 'all'}" for s, kind, sp, B, dt, f in CASES])
def test_operator_against_the_oracle(hip, size, kind, splat, B, dtype_name, filtered):
    Hp, Wp, H, W = size
    seed = Hp * 7 + W + B
    k = _calib()
    maps = _maps(Hp, Wp, B, seed)
    img = _image(B, H, W, dtype_name, seed)
    cam = _target(kind, H, W)
    reg = cloud.register(*(torch.from_numpy(a).cuda() for a in maps), torch.from_numpy(img).cuda(), to=cam, splat=splat, depth_trunc=3.0,
                         filtered=filtered, want_visible=True, **k)
    torch.cuda.synchronize()
    oracle = _oracle(maps, img, H, W, cam, splat, depth_trunc=3.0, filtered=filtered, **k)
    _check(reg, oracle, f"{kind} splat {splat}")
    covered = sum(o["count"] for o in oracle)
    print(f"[register] {W}x{H} -> {cam.width}x{cam.height} {kind} splat {splat} B={B}: {covered} of {B * cam.height * cam.width} target pixels covered")
    assert covered > 0
    if kind == "half":                               # really half outside: a part of the target stays empty, a part of the source is unseen
        assert covered < B * cam.height * cam.width and any((o["visible"] == 0)[o["keep"]].any() for o in oracle)
    # the NaN / +-inf disparities come out not kept: no target pixel names them, they are not visible
    vis, index = reg.visible.cpu().numpy(), reg.index.cpu().numpy()
    for b in range(B):
        bad = ~np.isfinite(cloud_oracle.crop(maps[0][b, 0], H, W))
        assert not vis[b, 0][bad].any() and not np.isin(index[b, 0], np.flatnonzero(bad.ravel())).any()


@pytest.mark.parametrize("trunc", [3.0, None])
def test_identity_target_returns_the_depth_map_of_k15(hip, trunc):
    """R = I, t = 0, cam0's intrinsics, the source's size, splat 1: every kept pixel lands on itself with Z = z bit for bit -- also the 1e6 m
    sentinel points of depth_trunc None.  The reference point is K15 itself (cloud.reproject) on the same inputs."""
    Hp, Wp, H, W = LARGE
    k = _calib()
    maps = tuple(torch.from_numpy(a).cuda() for a in _maps(Hp, Wp, 1, 77))
    img = torch.from_numpy(_image(1, H, W, "uint8", 77)).cuda()
    pc = cloud.reproject(*maps, img, depth_trunc=trunc, want_depth=True, want_mask=True, **k)
    reg = cloud.register(*maps, img, to=_target("identity", H, W), splat=1, depth_trunc=trunc, want_visible=True, **k)
    torch.cuda.synchronize()
    own = torch.arange(H * W, device="cuda", dtype=torch.int32).reshape(1, 1, H, W)
    kept = pc.mask.bool()
    assert torch.equal(reg.index, torch.where(kept, own, torch.full_like(own, -1)))
    assert torch.equal(reg.depth.view(torch.int32), pc.depth.view(torch.int32))
    assert torch.equal(reg.visible, pc.mask)
    assert torch.equal(reg.image, torch.where(kept, img, torch.zeros_like(img)))
    assert int(reg.count[0]) == int(kept.sum()) == int(pc.count[0]) and reg.holes(0) == H * W - int(pc.count[0])
    if trunc is None:
        assert bool((reg.depth == 1e6).any())


@pytest.mark.parametrize("H,W", [(24, 96), (64, 1216)])
def test_right_view_of_an_integer_disparity_scene(hip, H, W):
    """analytic, no oracle: a background at 8 px and a rectangle at 40 px seen from the rectified right camera (doffs = 0, cx1 = cx0: a pixel
    of disparity d lands d columns to the left).  The expectation is painted far to near (register_oracle.right_view_scene)."""
    k = dict(fx=1000.0, cx=50.0, cy=10.0, baseline=100.0, doffs=0.0)
    disp, index, visible = register_oracle.right_view_scene(H, W)
    calib = {"cam1": np.array([[1000.0, 0, 50.0], [0, 1000.0, 10.0], [0, 0, 1]]), "baseline": 100.0}
    one = torch.ones((1, 1, H, W), device="cuda")
    img = torch.from_numpy(_image(1, H, W, "uint8", 3)).cuda()
    reg = cloud.register(torch.from_numpy(disp).cuda().reshape(1, 1, H, W), one, one, img, to=cloud.right_camera(calib, W, H), splat=1,
                         want_visible=True, **k)
    torch.cuda.synchronize()
    assert np.array_equal(reg.index[0, 0].cpu().numpy(), index)
    assert np.array_equal(reg.visible[0, 0].cpu().numpy(), visible)
    # visible == 0 exactly on the background pixels that the rectangle hides or that leave the image
    r0, r1, c0, c1 = H // 4, 3 * H // 4, W // 2, 3 * W // 4
    hidden = np.zeros((H, W), dtype=bool)
    hidden[:, :8] = True
    hidden[r0:r1, c0 - 40 + 8:c1 - 40 + 8] = True
    hidden[r0:r1, c0:c1] = False
    assert np.array_equal(reg.visible[0, 0].cpu().numpy() == 0, hidden)
    # z = 100 / d m in the right camera too (a translation along x); colours follow the index
    z = np.where(index >= 0, F(1e5) / disp.ravel()[np.maximum(index, 0)] / F(1000.0), F(0)).astype(F)
    assert np.array_equal(reg.depth[0, 0].cpu().numpy(), z)
    want = np.where(index >= 0, img.cpu().numpy()[0].reshape(3, -1)[:, np.maximum(index, 0).ravel()].reshape(3, H, W), 0)
    assert np.array_equal(reg.image[0].cpu().numpy(), want)
    assert int(reg.count[0]) == int((index >= 0).sum())


def test_everything_onto_one_pixel(hip):
    """fx_t = fy_t = 1e-6: every kept pixel projects to (cx_t, cy_t) and 4096 atomic minima meet on one word.  The winner is the nearest Z and,
    among the two pixels that share it on purpose, the lower index"""
    H = W = 64
    k = _calib()
    disp, occ, conf = (a.copy() for a in _maps(H, W, 1, 9, False))
    flat = disp.reshape(-1)
    flat[[3001, 777]] = 310.0                                                        # the largest disparity of the map, twice: the nearest z
    assert flat.max() == 310.0 and (flat == 310.0).sum() == 2
    img = _image(1, H, W, "uint8", 9)
    cam = cloud.Camera(7, 5, 1e-6, 1e-6, 3.2, 2.4)
    reg = cloud.register(*(torch.from_numpy(a).cuda() for a in (disp, occ, conf)), torch.from_numpy(img).cuda(), to=cam, splat=1, filtered=False,
                         depth_trunc=3.0, want_visible=True, **k)
    torch.cuda.synchronize()
    z = F(F(k["baseline"] * k["fx"]) / (F(310.0) + F(k["doffs"]))) / F(1000.0)
    index = np.full((5, 7), -1, dtype=np.int32)
    index[2, 3] = 777                                                                # floor(3.2 + 0.5), floor(2.4 + 0.5)
    assert np.array_equal(reg.index[0, 0].cpu().numpy(), index)
    assert np.array_equal(reg.depth[0, 0].cpu().numpy(), np.where(index >= 0, z, F(0)).astype(F))
    vis = np.zeros(H * W, dtype=np.uint8)
    vis[777] = 1
    assert np.array_equal(reg.visible[0, 0].cpu().numpy().ravel(), vis)
    assert int(reg.count[0]) == 1 and reg.holes(0) == 34
    assert reg.image[0, :, 2, 3].cpu().tolist() == img[0].reshape(3, -1)[:, 777].tolist() and int(reg.image.sum()) == int(img[0].reshape(3, -1)[:, 777].sum())
    _check(reg, _oracle((disp, occ, conf), img, H, W, cam, 1, depth_trunc=3.0, filtered=False, **k), "one pixel")


@pytest.mark.parametrize("why", ["behind", "conf0"])
def test_nothing_lands(hip, why):
    """a target rotated by 180 degrees about y looks away from the scene (every Z < 0); a confidence of 0 keeps no pixel.  Either way: all holes,
    count 0, nothing visible -- written over whatever the output buffers held"""
    Hp, Wp, H, W = SMALL[1]
    B, k = 3, _calib()
    disp, occ, conf = (torch.from_numpy(a).cuda() for a in _maps(Hp, Wp, B, 31))
    if why == "conf0":
        conf = torch.zeros_like(conf)
    R = [-1, 0, 0, 0, 1, 0, 0, 0, -1] if why == "behind" else [1, 0, 0, 0, 1, 0, 0, 0, 1]
    img = torch.from_numpy(_image(B, H, W, "uint8", 31)).cuda()
    Ht, Wt = 48, 80
    out = dict(depth_t=torch.full((B, 1, Ht, Wt), 7.0, device="cuda"), index_t=torch.full((B, 1, Ht, Wt), PATTERN, device="cuda", dtype=torch.int32),
               image_t=torch.full((B, 3, Ht, Wt), 0x5A, device="cuda", dtype=torch.uint8),
               visible=torch.full((B, 1, H, W), 0x5A, device="cuda", dtype=torch.uint8), count=torch.full((B,), -7, device="cuda", dtype=torch.int32))
    ws = torch.empty(hip.register_workspace_bytes(B, Ht, Wt), device="cuda", dtype=torch.uint8)
    hip.register(disp, occ, conf, img, depth_trunc=3.0, Ht=Ht, Wt=Wt, splat=2, fx_t=k["fx"], fy_t=k["fy"], cx_t=k["cx"], cy_t=k["cy"], R=R, t=[0, 0, 0],
                 workspace=ws, **out, **k)
    torch.cuda.synchronize()
    assert bool((out["index_t"] == -1).all()) and bool((out["depth_t"].view(torch.int32) == 0).all())
    assert not bool(out["image_t"].any()) and not bool(out["visible"].any()) and out["count"].tolist() == [0] * B


def test_two_runs_are_byte_identical_also_on_poisoned_lds(hip):
    Hp, Wp, H, W = LARGE
    B, seed, k = 3, 41, _calib()
    maps = tuple(torch.from_numpy(a).cuda() for a in _maps(Hp, Wp, B, seed))
    img = torch.from_numpy(_image(B, H, W, "float16", seed)).cuda()
    cam = _target("rot", H, W)
    first = cloud.register(*maps, img, to=cam, splat=2, depth_trunc=3.0, want_visible=True, **k)
    torch.cuda.synchronize()
    hip.poison_lds()
    second = cloud.register(*maps, img, to=cam, splat=2, depth_trunc=3.0, want_visible=True, **k)
    torch.cuda.synchronize()
    assert int(first.count.min()) > 0
    for name in ("depth", "index", "image", "visible", "count"):
        a, b = getattr(first, name), getattr(second, name)
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.float32 else a, b.view(torch.uint8) if b.dtype == torch.float32 else b), name


def test_hipgraph_capture_and_replay_after_the_maps_change(hip):
    Hp, Wp, H, W = LARGE
    B, k = 1, _calib()
    draws = [tuple(a.copy() for a in _maps(Hp, Wp, B, s)) for s in (201, 202)]
    imgn = _image(B, H, W, "uint8", 201)
    img = torch.from_numpy(imgn).cuda()
    maps = tuple(torch.from_numpy(a).cuda() for a in draws[0])
    cam = _target("rot", H, W)
    Ht, Wt = cam.height, cam.width
    out = dict(depth_t=torch.zeros((B, 1, Ht, Wt), device="cuda"), index_t=torch.zeros((B, 1, Ht, Wt), device="cuda", dtype=torch.int32),
               image_t=torch.zeros((B, 3, Ht, Wt), device="cuda", dtype=torch.uint8), visible=torch.zeros((B, 1, H, W), device="cuda", dtype=torch.uint8),
               count=torch.zeros((B,), device="cuda", dtype=torch.int32))
    ws = torch.empty(hip.register_workspace_bytes(B, Ht, Wt), device="cuda", dtype=torch.uint8)
    kw = dict(depth_trunc=3.0, Ht=Ht, Wt=Wt, splat=2, fx_t=cam.fx, fy_t=cam.fy, cx_t=cam.cx, cy_t=cam.cy, R=cam.R.ravel().tolist(), t=cam.t.tolist(),
              workspace=ws, **out, **k)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.register(*maps, img, **kw)                           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hip.register(*maps, img, **kw)
    for d in draws:
        for t, a in zip(maps, d):
            t.copy_(torch.from_numpy(a))                         # in place: the graph keeps reading the same buffers
        for t in out.values():
            t.fill_(0x5A)
        ws.fill_(0x5A)                                           # the clear launch is part of the graph
        g.replay()
        torch.cuda.synchronize()
        reg = cloud.Registered(out["depth_t"], out["index_t"], out["image_t"], out["visible"], out["count"])
        o = _oracle(d, imgn, H, W, cam, 2, depth_trunc=3.0, **k)
        _check(reg, o, "replay")
    assert o[0]["count"] != 0


# ------------------------------------------------------------------------------------------------ end to end

def _s_model():
    from s2m2_amd.model import S2M2
    from s2m2_amd.spec import MODEL_CONFIGS
    from s2m2_amd.weights import seeded_state_dict
    C, ntr = MODEL_CONFIGS["S"]
    m = S2M2(C, 1, ntr, use_positivity=True, refine_iter=3)
    m.load_state_dict(seeded_state_dict(C, 1, ntr, 0), strict=True)
    return m.cuda().eval()


def test_forward_then_register(hip):
    from s2m2_amd import utils
    from s2m2_amd.weights import synthetic_pair
    H, W = 384, 512
    m = _s_model()
    left, right = synthetic_pair(H, W, 1, 24, 3)
    left_u8, right_u8 = left.to(torch.uint8).cuda(), right.to(torch.uint8).cuda()
    with torch.autocast("cuda", dtype=torch.float16):
        maps = [t.float().contiguous() for t in m(utils.image_pad(left_u8, 32), utils.image_pad(right_u8, 32))]
    torch.cuda.synchronize()
    k = _calib()
    cam = cloud.right_camera(cloud.read_calib_file(CALIB), W, H)
    host = tuple(t.cpu().numpy() for t in maps)
    imgn = left_u8.cpu().numpy()
    for filtered, trunc, splat in ((True, 3.0, 2), (False, None, 1)):
        reg = cloud.register(*maps, left_u8, to=cam, splat=splat, depth_trunc=trunc, filtered=filtered, want_visible=True, **k)
        torch.cuda.synchronize()
        o = _oracle(host, imgn, H, W, cam, splat, depth_trunc=trunc, filtered=filtered, **k)
        print(f"[register e2e] filtered={filtered} trunc={trunc} splat={splat}: {o[0]['count']} of {H * W} target pixels covered, "
              f"{int(o[0]['visible'].sum())} source pixels visible")
        _check(reg, o, "forward")


def test_runner_writes_the_registered_depth(hip, tmp_path):
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
    base = [RUNNER, path, str(tmp_path / "left.f32"), str(tmp_path / "right.f32")]
    k = _calib()
    calib = cloud.read_calib_file(CALIB)

    def run(tag, extra):
        out = tmp_path / tag
        out.mkdir()
        p = subprocess.run(base + ["--out", str(out)] + extra, capture_output=True, text=True, timeout=240)
        assert p.returncode == 0, p.stderr
        return out, p.stdout

    def maps_of(out):
        return [torch.from_numpy(np.fromfile(out / f"{n}.f32", dtype="<f4").reshape(1, 1, H, W)).cuda() for n in ("disp", "occ", "conf")]

    # the right view: colours from the engine's own float32 left input
    a, stdout = run("a", ["--calib", CALIB, "--depth-trunc", "3", "--register", "right", "--register-depth", str(tmp_path / "a.f32"),
                          "--register-image", str(tmp_path / "a.ppm"), "--register-index", str(tmp_path / "a.i32"), "--repeat", "2"])
    assert "register_us_per_pair" in stdout
    reg = cloud.register(*maps_of(a), left.cuda(), to=cloud.right_camera(calib, W, H), depth_trunc=3.0, **k)
    torch.cuda.synchronize()
    print(f"[register runner] right view: {int(reg.count[0])} target pixels covered")
    assert int(reg.count[0]) > 0
    assert (tmp_path / "a.f32").read_bytes() == reg.depth.cpu().numpy().tobytes()
    assert (tmp_path / "a.i32").read_bytes() == reg.index.cpu().numpy().tobytes()
    head = f"P6\n{W} {H}\n255\n".encode()
    assert (tmp_path / "a.ppm").read_bytes() == head + reg.image[0].permute(1, 2, 0).contiguous().cpu().numpy().tobytes()
    # a camera file: another size, a rotation and a translation, splat 3, next to --ply
    cam = cloud.Camera(320, 240, 2400.0, 2300.0, 700.5, 600.25, _rotation(1.0, -2.0, 0.5), (0.02, -0.01, 0.03))
    rows = lambda mat: "; ".join(" ".join(repr(float(x)) for x in r) for r in mat)
    (tmp_path / "cam.txt").write_text(f"width={cam.width}\nheight={cam.height}\ncam=[{cam.fx} 0 {cam.cx}; 0 {cam.fy} {cam.cy}; 0 0 1]\n"
                                      f"R=[{rows(cam.R)}]\nt=[{' '.join(repr(float(x)) for x in cam.t)}]\n")
    b, _ = run("b", ["--calib", CALIB, "--unfiltered", "--ply", str(tmp_path / "b.ply"), "--register", str(tmp_path / "cam.txt"), "--splat", "3",
                     "--register-depth", str(tmp_path / "b.f32")])
    reg = cloud.register(*maps_of(b), left.cuda(), to=cam, splat=3, filtered=False, **k)
    torch.cuda.synchronize()
    assert (tmp_path / "b.f32").read_bytes() == reg.depth.cpu().numpy().tobytes()
    pc = cloud.reproject(*maps_of(b), left.cuda(), filtered=False, **k)
    torch.cuda.synchronize()
    assert cloud.read_ply_records(str(tmp_path / "b.ply")).tobytes() == pc.records[0, :int(pc.count[0])].cpu().numpy().tobytes()
    # option errors are usage errors, before the engine is loaded
    for extra, msg in ((["--register", "right", "--register-depth", "x.f32"], "--register needs --calib and --register-depth"),
                       (["--calib", CALIB, "--register", "right"], "--register needs --calib and --register-depth"),
                       (["--calib", CALIB, "--ply", "x.ply", "--splat", "2"], "need --register"),
                       (["--calib", CALIB, "--register", "right", "--register-depth", "x.f32", "--splat", "5"], "--splat: 1, 2, 3 or 4")):
        p = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and msg in p.stderr, p.stderr
