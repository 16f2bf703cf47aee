"""K22 on the GPU (include/s2m2_hip.h: s2m2_segment; s2m2_amd/cloud.py: segment): connected components, sizes, the survivor mask, the padded
filtered disparity and the four counts against the numpy oracle of tests/segment_oracle.py -- never against the code under test.  Every
comparison is an equality over every pixel (floats as int32 bits): the label is the component's smallest raster index and the sizes are
integer sums, so nothing depends on the order in which the atomics arrive.

The shapes are built from the tile of the local pass (``hip.segment_tile``): TR x TC.  Most scenes run at (2 TR + 3) x (3 TC + 5) inside padded
maps with odd crop offsets, so that tile borders (which the crop offset shifts by ``ox & 3`` columns) cut every structure."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import cloud_oracle
import segment_oracle
from s2m2_amd import cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(ROOT, "tests", "golden", "bicycle2_calib.txt")
PATTERN = 0x5A5A5A5A
F = np.float32
INF = float("inf")
# z = 100 / d metres: with depth_trunc 1000 a pixel is kept iff conf and occ pass and d > 0.1
CAM = dict(fx=1000.0, fy=1000.0, cx=30.0, cy=20.0, baseline=100.0, doffs=0.0, depth_trunc=1000.0)


def _calib():
    c = cloud.read_calib_file(CALIB)
    return dict(fx=float(c["cam0"][0, 0]), fy=float(c["cam0"][1, 1]), cx=float(c["cam0"][0, 2]), cy=float(c["cam0"][1, 2]),
                baseline=float(c["baseline"]), doffs=float(c["doffs"]))


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


@pytest.fixture(scope="module")
def tile(hip):
    tr, tc = hip.segment_tile(1 << 12, 1 << 12)
    print(f"[segment] tile {tr} x {tc}")
    return tr, tc


def _pad(a, Hp, Wp, fill):
    """(B,H,W) -> (B,1,Hp,Wp) with the content as the centred crop and `fill` around it"""
    B, H, W = a.shape
    out = np.full((B, 1, Hp, Wp), fill, dtype=F)
    cloud_oracle.crop(out[:, 0], H, W)[...] = a
    return out


def _maps(disp, keep, pad=(0, 0)):
    """disp (B,H,W) float32 and keep (B,H,W) bool (kept through conf) -> padded maps; the border looks like kept pixels of disparity 10, which
    would join the image's if a kernel took them for image pixels"""
    disp, keep = np.asarray(disp, dtype=F), np.asarray(keep, dtype=bool)
    B, H, W = disp.shape
    Hp, Wp = H + pad[0], W + pad[1]
    return _pad(disp, Hp, Wp, 10.0), _pad(np.ones_like(disp), Hp, Wp, 1.0), _pad(keep.astype(F), Hp, Wp, 1.0)


def _dev(a, offset_floats=0):
    """a float32 array on the device; offset_floats: its first element that many floats behind a 256-byte boundary"""
    t = torch.empty(a.size + 64, dtype=torch.float32, device="cuda")
    assert t.data_ptr() % 256 == 0
    v = t[offset_floats:offset_floats + a.size].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return v


def _compare(s, maps, H, W, kw, tag=""):
    """a Segments against the oracle, pair by pair, every output"""
    disp, occ, conf = maps
    torch.cuda.synchronize()
    got = {k: getattr(s, k).cpu().numpy() for k in ("label", "size", "mask", "disp", "stats") if getattr(s, k) is not None}
    oracles = []
    for b in range(disp.shape[0]):
        with np.errstate(invalid="ignore"):
            o = segment_oracle.segment(cloud_oracle.crop(disp[b, 0], H, W), cloud_oracle.crop(occ[b, 0], H, W), cloud_oracle.crop(conf[b, 0], H, W),
                                       **{"fy": kw["fx"], **kw})
        oracles.append(o)
        print(f"[segment{tag}] pair {b}: {H}x{W} stats {o['stats'].tolist()} oracle sweeps {o['sweeps']}")
        if "label" in got:
            assert np.array_equal(got["label"][b, 0], o["label"])
        if "size" in got:
            assert np.array_equal(got["size"][b, 0], o["size"])
        assert np.array_equal(got["mask"][b, 0], o["mask"])
        assert np.array_equal(got["disp"][b, 0].view(np.int32), segment_oracle.disp_out(disp[b, 0], o["mask"], H, W).view(np.int32))
        assert got["stats"][b].tolist() == o["stats"].tolist()
    return oracles


def _run(maps, H, W, offset_floats=0, **kw):
    dev = [_dev(m, offset_floats) for m in maps]
    s = cloud.segment(*dev, H=H, W=W, **kw)
    return s, _compare(s, maps, H, W, kw)


# ---- scenes: (disp (H,W), keep (H,W), max_jump)

def _percolation(H, W, seed=0):
    return np.full((H, W), 10, F), np.random.default_rng(seed).random((H, W)) < 0.593, INF


def _serpentine(H, W):
    """full rows on every other line, joined alternately at the right and the left end: one component that crosses every vertical tile border
    on every second row"""
    k = np.zeros((H, W), bool)
    k[0::2] = True
    k[1::4, W - 1] = True
    k[3::4, 0] = True
    return np.full((H, W), 10, F), k, 0.0


def _spiral(H, W):
    """a rectangular spiral of one-pixel corridors two pixels apart, walked from the outer corner inwards: one component"""
    k = np.zeros((H, W), bool)
    top, left, bottom, right = 0, 0, H - 1, W - 1
    v, u = 0, 0
    k[0, 0] = True
    while top <= bottom and left <= right:
        for u in range(left, right + 1):
            k[top, u] = True
        for v in range(top, bottom + 1):
            k[v, right] = True
        if bottom - top < 2 or right - left < 2:
            break
        for u in range(right, left + 1, -1):
            k[bottom, u] = True
        k[bottom, left + 2] = True
        for v in range(bottom, top + 1, -1):
            k[v, left + 2] = True
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
        k[top, left] = True
    return np.full((H, W), 10, F), k, 0.0


def _comb(H, W):
    """teeth on every other column that meet only in the last row"""
    k = np.zeros((H, W), bool)
    k[:, 0::2] = True
    k[H - 1, :] = True
    return np.full((H, W), 10, F), k, 0.0


def _checkerboard(H, W):
    return np.full((H, W), 10, F), np.add.outer(np.arange(H), np.arange(W)) % 2 == 0, INF


def _all(H, W):
    return np.full((H, W), 10, F), np.ones((H, W), bool), 0.0


def _none(H, W):
    return np.full((H, W), 10, F), np.zeros((H, W), bool), INF


def _planes(H, W, seed=4):
    """vertical bands of planes with dyadic row slopes: 1 px per row (exactly max_jump 1: joined down the band), 1.25 (just above: every row of
    the band is a component of its own), 0 and 0.5; neighbouring bands are 0, exactly 1 or 64 px apart at their top.  On top, islands of 1 to
    12 pixels, each at a disparity 500 away from everything else, in a frame of dropped pixels"""
    g = np.random.default_rng(seed)
    d = np.empty((H, W), F)
    k = np.ones((H, W), bool)
    slopes, offsets = [1.0, 1.25, 0.0, 0.5], [0.0, 1.0, 64.0]
    edges = list(range(0, W, 23)) + [W]
    base = 100.0
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        base += offsets[i % 3]
        d[:, a:b] = (base + slopes[i % 4] * np.arange(H))[:, None]
    n = 1
    for _ in range(40):
        h, w = [(1, 1), (1, 2), (1, 3), (2, 2), (1, 5), (2, 3), (1, 7), (2, 4), (3, 3), (2, 5), (1, 11), (3, 4)][n - 1]
        if h + 2 > H or w + 2 > W:
            n = n % 12 + 1
            continue
        y, x = int(g.integers(0, H - h - 1)), int(g.integers(0, W - w - 1))
        k[y:y + h + 2, x:x + w + 2] = False
        k[y + 1:y + 1 + h, x + 1:x + 1 + w] = True
        d[y + 1:y + 1 + h, x + 1:x + 1 + w] = 900.0
        n = n % 12 + 1
    return d, k, 1.0


SCENES = dict(percolation=_percolation, serpentine=_serpentine, spiral=_spiral, comb=_comb, checkerboard=_checkerboard, all=_all, none=_none)


def test_oracle_sees_the_scenes_as_intended(tile):
    """(no GPU work: the structures that the cases below rely on are what they claim to be)"""
    tr, tc = tile
    H, W = 2 * tr + 3, 3 * tc + 5
    for name in ("serpentine", "spiral", "comb"):
        d, k, mj = SCENES[name](H, W)
        lab, size, _ = segment_oracle.components(k, d, mj)
        assert (lab[k] == 0).all() and (size[k] == k.sum()).all() and k.sum() > H * W // 4, name
    d, k, mj = _planes(H, W)
    lab, size, _ = segment_oracle.components(k, d, mj)
    sizes = set(size[k].tolist())
    assert set(range(1, 13)) <= sizes and max(sizes) > 13 * 2


# ---- the cases of the issue

@pytest.mark.parametrize("shape", ["1x1", "1xW", "Hx1"])
def test_degenerate_sizes(hip, tile, shape):
    tr, tc = tile
    H, W = dict([("1x1", (1, 1)), ("1xW", (1, 2 * tc + 3)), ("Hx1", (2 * tr + 3, 1))])[shape]
    g = np.random.default_rng(7)
    for keep in (np.ones((H, W), bool), g.random((H, W)) < 0.8, np.zeros((H, W), bool)):
        for pad in ((0, 0), (6, 10)):
            maps = _maps(np.full((1, H, W), 10, F), keep[None], pad)
            _run(maps, H, W, max_jump=0.0, min_size=2, **CAM)


@pytest.mark.parametrize("offset_floats", [0, 1])
def test_odd_crop_and_both_map_load_paths(hip, offset_floats):
    """37x53 in 64x64 maps: crop offsets (13, 5); maps on a 16-byte boundary (16-byte map loads) and 4 bytes behind one (per pixel)"""
    H, W = 37, 53
    d, k, mj = _percolation(H, W, seed=3)
    d = d + (np.random.default_rng(5).integers(0, 3, (H, W)) * 0.5).astype(F)           # steps of 0, 0.5 and 1
    maps = _maps(d[None], k[None], (64 - H, 64 - W))
    assert maps[0].shape == (1, 1, 64, 64)
    _run(maps, H, W, offset_floats, max_jump=0.5, min_size=4, **CAM)


def test_larger_than_one_tile_and_two_pairs(hip, tile):
    """(2 TR + 3) x (3 TC + 5), B = 2: pair 0 ends with a kept row and pair 1 starts with one, of the same disparity -- merged across the pair
    border, pair 1's labels and both pairs' sizes would change"""
    tr, tc = tile
    H, W = 2 * tr + 3, 3 * tc + 5
    d0, k0, _ = _percolation(H, W, seed=1)
    d1, k1, _ = _percolation(H, W, seed=2)
    k0[H - 1, :] = True
    k1[0, :] = True
    for pad in ((0, 0), (29, 27)):
        _, oracles = _run(_maps(np.stack([d0, d1]), np.stack([k0, k1]), pad), H, W, max_jump=INF, min_size=30, **CAM)
        assert oracles[0]["stats"].tolist() != oracles[1]["stats"].tolist()
        assert oracles[1]["label"][0, 0] == 0 and oracles[0]["label"][H - 1, 0] > 0


@pytest.mark.parametrize("pad", [(0, 0), (29, 27)], ids=["unpadded", "padded"])
@pytest.mark.parametrize("name", list(SCENES))
def test_scenes(hip, tile, name, pad):
    tr, tc = tile
    H, W = 2 * tr + 3, 3 * tc + 5
    d, k, mj = SCENES[name](H, W)
    _, oracles = _run(_maps(d[None], k[None], pad), H, W, max_jump=mj, min_size=3, **CAM)
    stats = oracles[0]["stats"].tolist()
    if name in ("serpentine", "spiral", "comb", "all"):
        assert stats == [int(k.sum()), 1, int(k.sum()), 1]
    if name == "all":
        assert stats[0] == H * W
    if name == "checkerboard":
        assert stats == [int(k.sum()), int(k.sum()), 0, 0]
    if name == "none":
        assert stats == [0, 0, 0, 0]


def test_planes_and_islands_with_every_min_size(hip, tile):
    tr, tc = tile
    H, W = 2 * tr + 3, 3 * tc + 5
    d, k, mj = _planes(H, W)
    maps = _maps(d[None], k[None], (29, 27))
    surviving = []
    for min_size in (1, 5, 13, H * W + 1):
        _, oracles = _run(maps, H, W, max_jump=mj, min_size=min_size, **CAM)
        surviving.append(int(oracles[0]["stats"][2]))
    assert surviving[0] > surviving[1] > surviving[2] > surviving[3] == 0


@functools.lru_cache(maxsize=1)
def _random_draw(B, Hp, Wp, seed):
    """the draw of test_hip_cloud.py -- disp uniform in [-20, 300], conf / occ uniform in [0, 1], values near a decision threshold moved away
    from it -- plus NaN, +inf and -inf disparities"""
    g = np.random.default_rng(seed)
    k = _calib()
    disp = (g.random((B, 1, Hp, Wp), dtype=F) * F(320.0) - F(20.0)).astype(F)
    conf, occ = g.random((B, 1, Hp, Wp), dtype=F), g.random((B, 1, Hp, Wp), dtype=F)
    t_trunc = k["baseline"] * k["fx"] / (3.0 * 1000.0) - k["doffs"]
    disp[(np.abs(disp) < 1e-3) | (np.abs(disp - t_trunc) < 1e-3)] = 100.0
    conf[np.abs(conf - 0.1) < 1e-6] = 0.2
    occ[np.abs(occ - 0.5) < 1e-6] = 0.6
    r = g.random(disp.shape)
    disp[r < 0.03] = np.nan
    disp[(r >= 0.03) & (r < 0.045)] = np.inf
    disp[(r >= 0.045) & (r < 0.06)] = -np.inf
    return disp, occ, conf


@pytest.mark.parametrize("filtered", [True, False])
@pytest.mark.parametrize("max_jump", [1.0, 60.0])
def test_random_draw_with_nan_and_inf(hip, tile, filtered, max_jump):
    tr, tc = tile
    H, W = 2 * tr + 3, 3 * tc + 5
    maps = _random_draw(2, H + 29, W + 27, 21)
    # noise: at max_jump 1 a joined edge is rare (2 px of a 320 px range) and pairs are the largest components to count on
    _, oracles = _run(maps, H, W, max_jump=max_jump, min_size=2 if max_jump == 1.0 else 4, filtered=filtered, depth_trunc=3.0, **_calib())
    assert 0 < oracles[0]["stats"][2] < oracles[0]["stats"][0]


def test_uninitialised_memory_second_call_and_dropped_outputs(hip, tile):
    """outputs and workspace pre-filled with 0x5A5A5A5A; a second call on the same workspace with other inputs; the optional outputs dropped
    one at a time: what is requested does not change, and the memory behind every output stays untouched"""
    tr, tc = tile
    H, W, B = 2 * tr + 3, 3 * tc + 5, 2
    Hp, Wp = H + 29, W + 27
    first = _random_draw(B, Hp, Wp, 21)
    d, k, _ = _planes(H, W)
    second = _maps(np.stack([d, d[::-1]]), np.stack([k, k[::-1]]), (29, 27))
    kw = dict(max_jump=1.0, min_size=6)
    cam = dict(depth_trunc=3.0, **_calib())
    n, guard = B * H * W, 64
    ws_bytes = hip.segment_workspace_bytes(B, H, W)

    def fresh(elems, dtype):
        t = torch.empty(elems + guard, dtype=dtype, device="cuda")
        t.view(torch.uint8).fill_(0x5A)
        return t

    ws = fresh(ws_bytes // 4, torch.int32)
    full = None
    for maps in (first, second):
        dev = [_dev(m) for m in maps]
        for drop in (None, "label", "size", "mask", "disp_out", "stats"):
            bufs = dict(label=fresh(n, torch.int32), size=fresh(n, torch.int32), mask=fresh(n, torch.uint8),
                        disp_out=fresh(B * Hp * Wp, torch.float32), stats=fresh(B * 4, torch.int32))
            shapes = dict(label=(B, 1, H, W), size=(B, 1, H, W), mask=(B, 1, H, W), disp_out=(B, 1, Hp, Wp), stats=(B, 4))
            outs = {name: (None if name == drop else t[:t.numel() - guard].view(shapes[name])) for name, t in bufs.items()}
            hip.segment(*dev, H=H, W=W, unfiltered=False, workspace=ws[:ws_bytes // 4].view(torch.uint8), **outs, **kw, **cam)
            torch.cuda.synchronize()
            for name, t in bufs.items():
                tail = t[t.numel() - guard:].view(torch.uint8)
                assert bool((tail == 0x5A).all()), f"memory behind {name} was written (dropped: {drop})"
                if name == drop:
                    assert bool((t.view(torch.uint8) == 0x5A).all())
            assert bool((ws[ws_bytes // 4:].view(torch.uint8) == 0x5A).all())
            if drop is None:
                s = cloud.Segments(outs["disp_out"], outs["mask"], outs["label"], outs["size"], outs["stats"])
                _compare(s, maps, H, W, dict(filtered=True, **kw, **cam), tag=" poisoned")
                full = {name: t.clone() for name, t in outs.items()}
            else:
                for name, t in outs.items():
                    if t is not None:
                        assert torch.equal(t, full[name]), f"{name} differs when {drop} is dropped"


def test_composition_with_the_cloud_and_the_mesh(hip, tile):
    """K15 on s.disp (filtered=False, depth_trunc 3) gives K15's own records restricted to s.mask; K20 on s.disp gives only faces inside one
    component, and with min_size 1 exactly K20's output on the original maps"""
    tr, tc = tile
    H, W, B = 2 * tr + 3, 3 * tc + 5, 2
    maps = _random_draw(B, H + 29, W + 27, 33)
    # more structure than noise: a smooth ramp (0.3 px per pixel, nearer than 3 m) on four pixels of five, confidence high on 85 % of the
    # pixels, so that the kept ramp pixels lie above the percolation threshold: one large component and many small ones
    g = np.random.default_rng(2)
    ramp = (100 + 0.3 * np.add.outer(np.arange(H + 29), np.arange(W + 27))).astype(F)
    with np.errstate(invalid="ignore"):
        disp = np.where(maps[0] > 40, ramp, maps[0]).astype(F)
    conf = np.where(g.random(disp.shape) < 0.85, F(0.9), F(0.05)).astype(F)
    dev = [_dev(m) for m in (disp, np.full_like(disp, 0.9), conf)]
    image = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (B, 3, H, W), dtype=np.uint8)).cuda()
    cam = dict(depth_trunc=3.0, **_calib())
    own = cloud.reproject(*dev, image, want_mask=True, **cam)
    own_mesh = cloud.mesh(*dev, image, max_jump=1.0, **cam)
    for min_size in (1, 9):
        s = cloud.segment(*dev, H=H, W=W, max_jump=1.0, min_size=min_size, **cam)
        pc = cloud.reproject(s.disp, dev[1], dev[2], image, filtered=False, want_mask=True, **cam)
        m = cloud.mesh(s.disp, dev[1], dev[2], image, filtered=False, max_jump=1.0, want_index=True, **cam)
        torch.cuda.synchronize()
        for b in range(B):
            mask = s.mask[b, 0].cpu().numpy().astype(bool)
            kept = own.mask[b, 0].cpu().numpy().astype(bool)
            assert not (mask & ~kept).any() and np.array_equal(pc.mask[b, 0].cpu().numpy().astype(bool), mask)
            records = own.records[b, :own.size(b)].cpu().numpy()[mask[kept]]
            assert pc.size(b) == int(mask.sum()) == s.surviving(b) and 0 < pc.size(b)
            assert np.array_equal(pc.records[b, :pc.size(b)].cpu().numpy(), records)
            # the faces: ranks -> pixels -> labels
            pixel = np.flatnonzero(mask.ravel())
            faces = m.faces(b).cpu().numpy()
            lab = s.label[b, 0].cpu().numpy().ravel()[pixel[faces]]
            assert len(faces) > 100 and (lab >= 0).all() and (lab[:, 0] == lab[:, 1]).all() and (lab[:, 1] == lab[:, 2]).all()
            if min_size == 1:
                assert np.array_equal(mask, kept) and s.kept(b) == s.surviving(b) and s.components(b) == s.surviving_components(b)
                assert np.array_equal(m.records[b, :m.size(b)].cpu().numpy(), own_mesh.records[b, :own_mesh.size(b)].cpu().numpy())
                assert np.array_equal(faces, own_mesh.faces(b).cpu().numpy())
            else:
                assert s.surviving(b) < s.kept(b) and s.surviving_components(b) < s.components(b)
                assert len(faces) <= own_mesh.face_size(b)


def test_two_eager_runs_and_a_graph_replay_are_byte_identical(hip, tile):
    tr, tc = tile
    H, W, B = 2 * tr + 3, 3 * tc + 5, 2
    maps = _random_draw(B, H + 29, W + 27, 21)
    dev = [_dev(m) for m in maps]
    kw = dict(H=H, W=W, max_jump=60.0, min_size=5, depth_trunc=3.0, **_calib())
    fields = ("disp", "mask", "label", "size", "stats")
    runs = []
    for _ in range(2):
        s = cloud.segment(*dev, **kw)
        torch.cuda.synchronize()
        runs.append([getattr(s, f).cpu().numpy().tobytes() for f in fields])
    assert runs[0] == runs[1]
    graph = torch.cuda.CUDAGraph()                           # (one stream, no side branches; the eager runs above were the warm-up)
    with torch.cuda.graph(graph):
        s = cloud.segment(*dev, **kw)
    for f in fields:
        getattr(s, f).view(torch.uint8).fill_(0x5A)
    graph.replay()
    torch.cuda.synchronize()
    assert [getattr(s, f).cpu().numpy().tobytes() for f in fields] == runs[0]


def test_filter_speckles_follows_get_pointcloud(hip):
    """utils.filter_speckles: halved intrinsics, no confidence filter, (H,W) in and out"""
    from s2m2_amd import utils
    H, W = 70, 90
    d, k, mj = _planes(H, W, seed=9)
    disp = np.where(k, d, F(-1.0)).astype(F)
    calib = cloud.read_calib_file(CALIB)
    out = utils.filter_speckles(disp, calib, depth_trunc=50.0, max_jump=1.0, min_size=13)
    c = _calib()
    o = segment_oracle.segment(disp, disp, disp, fx=c["fx"] / 2.0, fy=c["fx"] / 2.0, cx=c["cx"] / 2.0, cy=c["cy"] / 2.0, baseline=c["baseline"],
                               doffs=c["doffs"], depth_trunc=50.0, filtered=False, max_jump=1.0, min_size=13)
    assert out.shape == (H, W) and out.is_cuda and 0 < o["stats"][2] < o["stats"][0]
    assert np.array_equal(out.cpu().numpy().view(np.int32), np.where(o["mask"].astype(bool), disp, F(-1.0)).view(np.int32))


@functools.lru_cache(maxsize=1)
def _s_model():
    from s2m2_amd.model import S2M2
    from s2m2_amd.spec import MODEL_CONFIGS
    from s2m2_amd.weights import seeded_state_dict
    C, ntr = MODEL_CONFIGS["S"]
    m = S2M2(C, 1, ntr, use_positivity=True, refine_iter=3)
    m.load_state_dict(seeded_state_dict(C, 1, ntr, 0), strict=True)
    return m.cuda().eval()


def test_runner_filters_in_front_of_the_3d_outputs(hip, tmp_path):
    from s2m2_amd.build import RUNNER
    from s2m2_amd.export import export_engine
    from s2m2_amd.weights import synthetic_pair
    H, W = 384, 512
    path = str(tmp_path / "s_384x512.s2m2")
    export_engine(_s_model(), path, H, W)
    left, right = synthetic_pair(H, W, 1, 24, 11)
    left, right = left.contiguous(), right.contiguous()
    (tmp_path / "left.f32").write_bytes(left.numpy().astype("<f4").tobytes())
    (tmp_path / "right.f32").write_bytes(right.numpy().astype("<f4").tobytes())
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

    common = ["--calib", CALIB, "--depth-trunc", "3", "--conf-min", "0.02", "--max-jump", "inf"]
    a, stdout = run("a", common + ["--min-size", "2", "--ply", str(tmp_path / "a.ply"), "--mesh", str(tmp_path / "a_mesh.ply"),
                                   "--labels", str(tmp_path / "a.i32"), "--segment-mask", str(tmp_path / "a.u8"), "--repeat", "2"])
    assert "segment_us_per_pair" in stdout and "segment_components" in stdout
    # --repeat: one JSON line per timed stage, in the order forward, segment, mesh, cloud, each with exactly its keys
    assert [set(json.loads(line)) for line in stdout.splitlines()] == [
        {"B", "H", "W", "repeat", "ms_per_pair"},
        {"segment_kept", "segment_components", "segment_surviving", "repeat", "segment_us_per_pair"},
        {"mesh_vertices", "mesh_faces", "repeat", "mesh_us_per_pair"},
        {"cloud_points", "repeat", "cloud_us_per_pair"}], stdout
    maps = maps_of(a)
    kw = dict(depth_trunc=3.0, conf_min=0.02, **k)
    s = cloud.segment(*maps, H=H, W=W, max_jump=INF, min_size=2, **kw)
    pc = cloud.reproject(s.disp, maps[1], maps[2], left.cuda(), filtered=False, **kw)
    m = cloud.mesh(s.disp, maps[1], maps[2], left.cuda(), filtered=False, max_jump=INF, **kw)
    torch.cuda.synchronize()
    print(f"[segment runner] stats {s.stats[0].tolist()}")
    assert 0 < s.surviving(0) < s.kept(0)        # (a seeded model's maps: the kept pixels are sparse, singletons go and pairs stay)
    assert (tmp_path / "a.i32").read_bytes() == s.label.cpu().numpy().tobytes()
    assert (tmp_path / "a.u8").read_bytes() == s.mask.cpu().numpy().tobytes()
    assert cloud.read_ply_records(str(tmp_path / "a.ply")).tobytes() == pc.records[0, :pc.size(0)].cpu().numpy().tobytes()
    rec, faces = cloud.read_ply_mesh(str(tmp_path / "a_mesh.ply"))
    assert rec.tobytes() == m.records[0, :m.size(0)].cpu().numpy().tobytes() and np.array_equal(faces, m.faces(0).cpu().numpy())
    # without --min-size: today's files
    b, _ = run("b", common + ["--ply", str(tmp_path / "b.ply"), "--mesh", str(tmp_path / "b_mesh.ply")])
    maps = maps_of(b)
    pc = cloud.reproject(*maps, left.cuda(), **kw)
    m = cloud.mesh(*maps, left.cuda(), max_jump=INF, **kw)
    torch.cuda.synchronize()
    assert cloud.read_ply_records(str(tmp_path / "b.ply")).tobytes() == pc.records[0, :pc.size(0)].cpu().numpy().tobytes()
    rec, faces = cloud.read_ply_mesh(str(tmp_path / "b_mesh.ply"))
    assert rec.tobytes() == m.records[0, :m.size(0)].cpu().numpy().tobytes() and np.array_equal(faces, m.faces(0).cpu().numpy())
    assert pc.size(0) >= s.surviving(0)
