"""K23 on the GPU (include/s2m2_hip.h: s2m2_voxel; s2m2_amd/cloud.py: voxelize): the voxel records, weights, count, index and stats against the
numpy oracle of tests/voxel_oracle.py -- never against the code under test.  Every comparison is an equality (floats as int32 bits, every
record, every output): the aggregates are integer sums and minima and the records are ordered by raster rank, so nothing depends on the
order in which the atomics arrive.

Two kinds of scene.  "Plane" scenes use an ordinary camera, so that voxels are patches of pixels that straddle tile and wave borders.  "Cell"
scenes use a camera with a very long focal length and the principal point outside the image (x and y are tiny and positive: ix = iy = 0), so
that a pixel's voxel is chosen through its disparity alone: iz = the cell the test asks for.  What a scene is meant to contain is asserted
from the oracle's voxel list before anything is compared."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import cloud_oracle
import voxel_oracle
from s2m2_amd import cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(ROOT, "tests", "golden", "bicycle2_calib.txt")
F = np.float32
# plane scenes: z = 100 / d metres
CAM = dict(fx=1000.0, fy=1000.0, cx=33.0, cy=40.0, baseline=100.0, doffs=0.0, depth_trunc=1000.0)
# cell scenes: z = 100 / d, x = (u + 8) * z * 1e-6, y likewise; with CELL_SIZE the cell of a pixel is (0, 0, iz), z = (iz + 0.5) * CELL_SIZE
CELL_CAM = dict(fx=1e6, fy=1e6, cx=-8.0, cy=-8.0, baseline=1e-4, doffs=0.0, depth_scale=1.0, depth_trunc=1e6)
CELL_SIZE = 0.5


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
    """rows of a raster tile at W = 67"""
    rows = hip.voxel_tile_rows(1 << 12, 67)
    print(f"[voxel] {rows} rows per tile at W = 67")
    return rows


def _pad(a, Hp, Wp, fill):
    B, H, W = a.shape
    out = np.full((B, 1, Hp, Wp), fill, dtype=F)
    cloud_oracle.crop(out[:, 0], H, W)[...] = a
    return out


def _maps(disp, keep=None, pad=(0, 0)):
    """disp (B,H,W) and keep (B,H,W) bool (dropped through conf) -> padded maps; the border holds kept pixels of disparity 10, which would
    add voxels if a kernel took them for image pixels"""
    disp = np.asarray(disp, dtype=F)
    keep = np.ones(disp.shape, bool) if keep is None else np.asarray(keep, dtype=bool)
    B, H, W = disp.shape
    Hp, Wp = H + pad[0], W + pad[1]
    return _pad(disp, Hp, Wp, 10.0), _pad(np.ones_like(disp), Hp, Wp, 1.0), _pad(keep.astype(F), Hp, Wp, 1.0)


def _cell_disp(cells):
    """the disparity that puts a pixel of a cell scene into cell iz (the middle of the cell)"""
    return (F(100.0) / ((np.asarray(cells, dtype=np.float64) + 0.5) * CELL_SIZE)).astype(F)


def _image(B, H, W, seed=1, dtype=np.uint8):
    g = np.random.default_rng(seed)
    if dtype == np.uint8:
        return g.integers(0, 256, (B, 3, H, W), dtype=np.uint8)
    return (g.random((B, 3, H, W)) * 280.0 - 10.0).astype(dtype)            # beyond [0, 255] on both sides: clamped


def _dev(a, offset_floats=0):
    t = torch.empty(a.size + 64, dtype=torch.float32, device="cuda")
    assert t.data_ptr() % 256 == 0
    v = t[offset_floats:offset_floats + a.size].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return v


def _oracles(maps, image, kw):
    H, W = image.shape[-2:]
    out = []
    for b in range(image.shape[0]):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            out.append(voxel_oracle.voxelize(*(cloud_oracle.crop(m[b, 0], H, W) for m in maps), image[b], **{"fy": kw["fx"], **kw}))
    return out


def _compare(vc, oracles, tag=""):
    torch.cuda.synchronize()
    count, stats = vc.count.cpu().numpy(), vc.stats.cpu().numpy()
    for b, o in enumerate(oracles):
        n = len(o["records"])
        print(f"[voxel{tag}] pair {b}: stats {o['stats'].tolist()} largest voxel {int(o['weights'].max()) if n else 0}")
        assert stats[b].tolist() == o["stats"].tolist()
        assert count[b] == n and n <= vc.capacity
        assert np.array_equal(vc.records[b, :n].cpu().numpy(), o["records"])
        if vc.weights_buf is not None:
            assert np.array_equal(vc.weights_buf[b, :n].cpu().numpy(), o["weights"])
        if vc.index is not None:
            assert np.array_equal(vc.index[b, 0].cpu().numpy(), o["index"])


def _run(maps, image, offset_floats=0, want_index=True, oracles=None, **kw):
    dev = [_dev(m, offset_floats) for m in maps]
    vc = cloud.voxelize(*dev, torch.from_numpy(image).cuda(), want_index=want_index, **kw)
    oracles = _oracles(maps, image, kw_oracle(kw)) if oracles is None else oracles
    _compare(vc, oracles)
    return vc, oracles


def kw_oracle(kw):
    return {k: v for k, v in kw.items() if k not in ("max_voxels", "capacity", "want_weights")}


# ---- the library without run combining (an experiment build: S2M2_LIB_SUFFIX=_voxel_plain S2M2_BUILD_DEFINES=-DS2M2_VOXEL_COMBINE=0)

@functools.lru_cache(maxsize=1)
def _plain_library():
    from s2m2_amd import hip as h
    path = h.LIB_PATH.replace(".so", "_voxel_plain.so")
    if not os.path.exists(path):
        return None
    lib = ctypes.CDLL(path)
    for name, (res, args) in h.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


@pytest.fixture(params=["combined", "plain"])
def build(request, hip, monkeypatch):
    """the shipped library, and the build with one insertion per point where it exists on the box"""
    if request.param == "plain":
        lib = _plain_library()
        if lib is None:
            pytest.skip("no build without run combining on this box (libs2m2_hip_voxel_plain.so)")
        monkeypatch.setattr(hip, "_lib", lib)
    return request.param


# ---- tile and wave borders

def _slanted(H, W, seed):
    """a plane that recedes along both axes, with a few far steps: about 5 x 5 pixels per 0.05 m voxel at 10 m"""
    g = np.random.default_rng(seed)
    z = 9.0 + 0.004 * np.arange(W)[None, :] + 0.003 * np.arange(H)[:, None] + (g.random((H, W)) < 0.02) * 3.0
    return (100.0 / z).astype(F), g.random((H, W)) < 0.9


@pytest.mark.parametrize("offset_floats", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("pad", [(0, 0), (29, 27)], ids=["unpadded", "odd-crop"])
def test_slanted_plane_over_tile_and_wave_borders(hip, tile, build, pad, offset_floats):
    H, W, B = 3 * tile + 7, 67, 2
    scenes = [_slanted(H, W, s) for s in (1, 2)]
    maps = _maps(np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes]), pad)
    image = _image(B, H, W)
    _, oracles = _run(maps, image, offset_floats, voxel_size=0.05, **CAM)
    for o in oracles:
        assert 6 < o["stats"][0] / o["stats"][3] < 40 and o["stats"][1] == 0
        rows = o["first"] // W
        assert len(np.unique(rows // tile)) == 4                      # leaders in every tile, the partial one included
    assert oracles[0]["stats"].tolist() != oracles[1]["stats"].tolist()


# ---- runs

def _runs_scene():
    H, W = 4, 640
    cells = np.zeros((H, W), np.int64)
    keep = np.ones((H, W), bool)
    cells[0, :300] = 5                                           # one voxel over 300 consecutive pixels: longer than a wave's 256
    cells[0, 300:364] = 100 + np.arange(64)                      # runs of length 1
    cells[0, 364:492] = 7 + (np.arange(128) % 2)                 # A B A B
    cells[0, 492:] = 9
    cells[1] = 20 + np.arange(W) // 37                           # runs of 37, cut by dropped pixels
    keep[1, 100:300:5] = False
    keep[1, 400:420] = False
    cells[2, :600] = 300 + np.arange(600) // 3
    cells[2, 600:] = 250                                         # ends the row ...
    cells[3, :40] = 250                                          # ... and the next row begins in the same voxel
    cells[3, 40:] = 600 + np.arange(W - 40) // 150
    return cells, keep


@pytest.mark.parametrize("pad", [(0, 0), (6, 10)], ids=["unpadded", "odd-crop"])
def test_runs(hip, build, pad):
    cells, keep = _runs_scene()
    H, W = cells.shape
    maps = _maps(_cell_disp(cells)[None], keep[None], pad)
    image = _image(1, H, W, seed=3)
    _, (o,) = _run(maps, image, voxel_size=CELL_SIZE, **CELL_CAM)
    want = np.unique(cells[keep])
    assert (o["voxels"][:, :2] == 0).all() and sorted(o["voxels"][:, 2].tolist()) == want.tolist()
    by_cell = dict(zip(o["voxels"][:, 2].tolist(), o["weights"].tolist()))
    assert by_cell[5] == 300 and by_cell[7] == 64 and by_cell[8] == 64 and by_cell[250] == 80 and by_cell[100] == 1
    assert by_cell[22] < 37                                          # cut by dropped pixels


# ---- contention and accumulator width

def test_one_voxel_far_from_the_origin(hip, build):
    H, W = 200, 200
    cells = np.full((H, W), 2000, np.int64)                          # z = 1000.25: X, Y up to 400, Z about 2^21
    maps = _maps(_cell_disp(cells)[None])
    image = np.full((1, 3, H, W), 255, np.uint8)
    image[0, 1] = 254
    _, (o,) = _run(maps, image, voxel_size=CELL_SIZE, **CELL_CAM)
    assert o["stats"].tolist() == [H * W, 0, 0, 1] and o["weights"].tolist() == [H * W]
    assert o["records"][0, 3:].view(np.uint8).tolist() == [255, 254, 255, 255]


def test_every_pixel_its_own_voxel_at_load_one_half(hip, build):
    H, W = 48, 67
    cells = np.random.default_rng(5).permutation(H * W).reshape(H, W) * 3 + 10
    maps = _maps(_cell_disp(cells)[None], None, (5, 9))
    image = _image(1, H, W, seed=4)
    vc, (o,) = _run(maps, image, voxel_size=CELL_SIZE, max_voxels=H * W, capacity=H * W, **CELL_CAM)
    assert o["stats"].tolist() == [H * W, 0, 0, H * W] and vc.complete(0)
    assert np.array_equal(o["index"].ravel(), np.arange(H * W))


# ---- probing

@functools.lru_cache(maxsize=1)
def _probing_scene():
    """30 cells in a table of 64 slots, the seed searched until three of them share a home slot and linear probing wraps past the last slot"""
    from s2m2_amd import hip as h
    for seed in range(2000):
        g = np.random.default_rng(seed)
        chosen = g.choice(np.arange(10, 5000), 30, replace=False)
        home = np.array([h.voxel_home_slot(0, 0, int(c), 64) for c in chosen])
        if np.bincount(home, minlength=64).max() >= 3 and _wraps(home):
            H, W = 20, 30
            return chosen[g.integers(0, 30, (H, W))], seed
    raise AssertionError("no seed found")


def _wraps(home):
    """linear probing of these home slots into 64 slots, in the order given: does a key land below its home?  (Whether ANY key wraps does not
    depend on the order: the set of occupied slots does not.)"""
    taken = set()
    wrapped = False
    for s in home.tolist():
        t = s
        while t % 64 in taken:
            t += 1
        taken.add(t % 64)
        wrapped |= t >= 64
    return wrapped


def test_probe_chains_in_a_table_of_64_slots(hip, build):
    cells, seed = _probing_scene()
    H, W = cells.shape
    maps = _maps(_cell_disp(cells)[None])
    image = _image(1, H, W, seed=6)
    o = _oracles(maps, image, dict(voxel_size=CELL_SIZE, **CELL_CAM))
    # the preconditions, from the oracle's voxel list
    voxels = o[0]["voxels"]
    home = np.array([hip.voxel_home_slot(int(a), int(b), int(c), 64) for a, b, c in voxels])
    assert hip.voxel_slots(32) == 64 and len(voxels) <= 32 and np.bincount(home, minlength=64).max() >= 3 and _wraps(home)
    print(f"[voxel probing] seed {seed}: {len(voxels)} voxels, busiest home slot holds {np.bincount(home).max()}")
    vc, _ = _run(maps, image, voxel_size=CELL_SIZE, max_voxels=32, capacity=32, oracles=o, **CELL_CAM)
    assert vc.complete(0)


# ---- full table

def test_full_table_returns_and_reports(hip, build):
    H, W = 24, 67
    cells = 10 + np.random.default_rng(8).integers(0, 500, (H, W))
    maps = _maps(_cell_disp(cells)[None])
    image = _image(1, H, W)
    dev = [_dev(m) for m in maps]
    vc = cloud.voxelize(*dev, torch.from_numpy(image).cuda(), voxel_size=CELL_SIZE, max_voxels=32, capacity=64, want_index=True, **CELL_CAM)
    torch.cuda.synchronize()
    stats = vc.stats[0].tolist()
    distinct = len(np.unique(cells))
    assert distinct > 450 and stats[0] == H * W and stats[1] == 0
    assert stats[2] > 0 and not vc.complete(0)
    assert 0 < stats[3] <= hip.voxel_slots(32) == 64 and int(vc.count[0]) == stats[3]


# ---- a table that just fits, with every block of a full-size image racing for the same new voxels

@functools.lru_cache(maxsize=1)
def _racing_scene():
    """1216x1024, a slanted plane in 0.2 m voxels: a few thousand voxels, each claimed at once by the run heads of many rows and blocks"""
    H, W = 1024, 1216
    d, k = _slanted(H, W, 11)
    maps = _maps(d[None], k[None])
    image = _image(1, H, W, seed=12)
    kw = dict(voxel_size=0.2, **CAM)
    return maps, image, kw, _oracles(maps, image, kw)


@pytest.mark.parametrize("room", [0, 7], ids=["exactly", "seven-spare"])
def test_a_table_that_just_fits_never_drops_a_point(hip, build, room):
    """max_voxels equal to the number of distinct voxels, and slightly above it: no point is dropped and every record is the oracle's,
    although all blocks of the image start on an empty table together and thousands of insertions race for each new voxel"""
    maps, image, kw, oracles = _racing_scene()
    n = int(oracles[0]["stats"][3])
    assert 2000 < n < 20000 and oracles[0]["stats"][0] > 1000000
    vc, _ = _run(maps, image, oracles=oracles, max_voxels=n + room, capacity=n + room, **kw)
    assert vc.complete(0) and int(vc.stats[0, 2]) == 0


def test_one_voxel_with_max_voxels_one(hip, build):
    """a table of two slots for an image that is one voxel: every wave races for the one claim, one wins, nobody is refused"""
    H, W = 200, 200
    cells = np.full((H, W), 2000, np.int64)
    maps = _maps(_cell_disp(cells)[None])
    image = _image(1, H, W, seed=13)
    vc, (o,) = _run(maps, image, voxel_size=CELL_SIZE, max_voxels=1, capacity=1, **CELL_CAM)
    assert o["stats"].tolist() == [H * W, 0, 0, 1] and vc.complete(0)


# ---- range

def test_dropped_out_of_range_and_all_four_quadrants(hip, build):
    """depth_trunc None keeps d <= 0 at z = 1e6: out of range at this voxel size; the principal point in the middle of the image"""
    H, W = 37, 53
    g = np.random.default_rng(9)
    disp = (g.random((1, H, W), dtype=F) * F(30.0) + F(5.0)).astype(F)
    disp[g.random(disp.shape) < 0.1] = -1.0
    disp[0, 5, 7] = 0.0
    maps = _maps(disp, g.random(disp.shape) < 0.9, (11, 11))
    cam = dict(fx=500.0, cx=26.0, cy=18.0, baseline=100.0, doffs=0.0, depth_trunc=None)
    _, (o,) = _run(maps, _image(1, H, W), voxel_size=0.02, max_voxels=H * W, capacity=H * W, **cam)        # (more voxels than the default H * W / 4)
    assert o["stats"][1] > 50 and o["stats"][3] > 200
    signs = {(int(np.sign(a + 0.5)), int(np.sign(b + 0.5))) for a, b in o["voxels"][:, :2]}
    assert signs == {(-1, -1), (-1, 1), (1, -1), (1, 1)}


# ---- contract details

def test_capacity_below_count_poisoned_memory_dtypes_and_two_calls(hip):
    """records and weights beyond capacity, the memory behind every output and the workspace's surroundings stay 0x5A; a workspace full of
    0x5A changes nothing; a second call gives the same bytes; uint8, fp16 and fp32 images give the records of their rounded bytes"""
    H, W, B = 70, 67, 2
    scenes = [_slanted(H, W, s) for s in (3, 4)]
    maps = _maps(np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes]), (3, 5))
    dev = [_dev(m) for m in maps]
    kw = dict(voxel_size=0.05, **CAM)
    mv = H * W // 4
    guard = 64
    ws_bytes = hip.voxel_workspace_bytes(B, H, W, mv)

    def fresh(elems, dtype=torch.int32):
        t = torch.empty(elems + guard, dtype=dtype, device="cuda")
        t.view(torch.uint8).fill_(0x5A)
        return t

    for dtype in (np.uint8, np.float16, np.float32):
        image = _image(B, H, W, seed=7, dtype=dtype)
        oracles = _oracles(maps, image, kw)
        full = min(len(o["records"]) for o in oracles)
        assert full > 40
        for cap in (mv, full - 17):
            runs = []
            for _ in range(2):
                ws = fresh(ws_bytes // 4)
                bufs = dict(records=fresh(B * cap * 4), weights=fresh(B * cap), count=fresh(B), index=fresh(B * H * W), stats=fresh(B * 4))
                shapes = dict(records=(B, cap, 4), weights=(B, cap), count=(B,), index=(B, 1, H, W), stats=(B, 4))
                outs = {k: t[:t.numel() - guard].view(shapes[k]) for k, t in bufs.items()}
                hip.voxel(*dev, torch.from_numpy(image).cuda(), fy=CAM["fx"], **{k: v for k, v in CAM.items() if k != "fy"}, voxel_size=0.05,
                          max_voxels=mv, workspace=ws[:ws_bytes // 4].view(torch.uint8), **outs)
                torch.cuda.synchronize()
                for k, t in bufs.items():
                    assert bool((t[t.numel() - guard:].view(torch.uint8) == 0x5A).all()), f"memory behind {k} was written"
                assert bool((ws[ws_bytes // 4:].view(torch.uint8) == 0x5A).all())
                for b, o in enumerate(oracles):
                    n = len(o["records"])
                    assert int(outs["count"][b]) == n and outs["stats"][b].tolist() == o["stats"].tolist()      # the true count above capacity
                    assert np.array_equal(outs["records"][b, :min(n, cap)].cpu().numpy(), o["records"][:cap])
                    assert np.array_equal(outs["weights"][b, :min(n, cap)].cpu().numpy(), o["weights"][:cap])
                    assert bool((outs["records"][b, min(n, cap):].view(torch.uint8) == 0x5A).all())
                    assert bool((outs["weights"][b, min(n, cap):].view(torch.uint8) == 0x5A).all())
                    assert np.array_equal(outs["index"][b, 0].cpu().numpy(), o["index"])                        # true ranks, also >= capacity
                    # weights sum to kept minus dropped; a bincount of index equals weights
                    assert int(o["weights"].sum()) == o["stats"][0] - o["stats"][1] - o["stats"][2]
                    idx = outs["index"][b].cpu().numpy().ravel()
                    assert np.array_equal(np.bincount(idx[idx >= 0], minlength=n), o["weights"])
                runs.append([t.cpu().numpy().tobytes() for t in bufs.values()])
            assert runs[0] == runs[1]


def test_outputs_dropped_one_at_a_time(hip):
    H, W, B = 40, 67, 1
    d, k = _slanted(H, W, 5)
    maps = _maps(d[None], k[None])
    dev = [_dev(m) for m in maps]
    image = torch.from_numpy(_image(B, H, W)).cuda()
    mv = H * W // 4
    ws = torch.empty(hip.voxel_workspace_bytes(B, H, W, mv), dtype=torch.uint8, device="cuda")
    make = dict(records=lambda: torch.zeros(B, mv, 4, dtype=torch.int32, device="cuda"), weights=lambda: torch.zeros(B, mv, dtype=torch.int32, device="cuda"),
                count=lambda: torch.zeros(B, dtype=torch.int32, device="cuda"), index=lambda: torch.zeros(B, 1, H, W, dtype=torch.int32, device="cuda"),
                stats=lambda: torch.zeros(B, 4, dtype=torch.int32, device="cuda"))
    full = None
    for drop in (None, "records", "weights", "count", "index", "stats"):
        outs = {k: (None if k == drop else f()) for k, f in make.items()}
        hip.voxel(*dev, image, fy=CAM["fx"], **CAM_NO_FY, voxel_size=0.05, max_voxels=mv, workspace=ws, **outs)
        torch.cuda.synchronize()
        if drop is None:
            full = outs
            assert int(full["count"][0]) > 50
        else:
            for k, t in outs.items():
                if t is not None:
                    assert torch.equal(t, full[k]), f"{k} differs when {drop} is dropped"


CAM_NO_FY = {k: v for k, v in CAM.items() if k != "fy"}


def test_two_eager_runs_and_a_graph_replay_are_byte_identical(hip):
    H, W, B = 70, 67, 2
    scenes = [_slanted(H, W, s) for s in (6, 7)]
    maps = _maps(np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes]), (29, 27))
    dev = [_dev(m) for m in maps]
    image_np = _image(B, H, W)
    image = torch.from_numpy(image_np).cuda()
    kw = dict(voxel_size=0.05, want_index=True, **CAM)
    fields = ("records", "weights_buf", "count", "index", "stats")
    oracles = _oracles(maps, image_np, dict(voxel_size=0.05, **CAM))

    def stored(vc):
        n = [int(c) for c in vc.count.cpu()]
        return [vc.records[b, :n[b]].cpu().numpy().tobytes() + vc.weights_buf[b, :n[b]].cpu().numpy().tobytes() for b in range(B)] + \
               [getattr(vc, f).cpu().numpy().tobytes() for f in ("count", "index", "stats")]

    runs = []
    for _ in range(2):
        vc = cloud.voxelize(*dev, image, **kw)
        _compare(vc, oracles)
        runs.append(stored(vc))
    assert runs[0] == runs[1]
    graph = torch.cuda.CUDAGraph()                           # (one stream, no side branches; the eager runs above were the warm-up)
    with torch.cuda.graph(graph):
        vc = cloud.voxelize(*dev, image, **kw)
    for _ in range(2):
        for f in fields:
            getattr(vc, f).view(torch.uint8).fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        assert stored(vc) == runs[0]


def test_voxelize_behind_segment(hip):
    """K22's filtered map with filtered=False: exactly the voxels of the surviving pixels"""
    H, W = 70, 67
    d, k = _slanted(H, W, 8)
    maps = _maps(d[None], k[None], (29, 27))
    dev = [_dev(m) for m in maps]
    image_np = _image(1, H, W)
    s = cloud.segment(*dev, H=H, W=W, max_jump=0.25, min_size=6, **CAM)
    vc = cloud.voxelize(s.disp, dev[1], dev[2], torch.from_numpy(image_np).cuda(), filtered=False, voxel_size=0.05, want_index=True, **CAM)
    torch.cuda.synchronize()
    assert 0 < s.surviving(0) < s.kept(0)
    filtered = s.disp.cpu().numpy()
    _compare(vc, _oracles((filtered, maps[1], maps[2]), image_np, dict(voxel_size=0.05, filtered=False, **CAM)), tag=" behind segment")
    assert int(vc.stats[0, 0]) == s.surviving(0)
    assert np.array_equal(vc.index[0, 0].cpu().numpy() >= 0, s.mask[0, 0].cpu().numpy().astype(bool))


def test_voxel_down_sample_follows_get_pointcloud(hip):
    """utils.voxel_down_sample: halved intrinsics, fx for both focal lengths, no confidence filter, (H,W,3) colours"""
    from s2m2_amd import utils
    H, W = 70, 90
    g = np.random.default_rng(10)
    disp = (60.0 + 0.2 * np.add.outer(np.arange(H), np.arange(W)) + g.random((H, W))).astype(F)
    disp[g.random((H, W)) < 0.1] = -1.0
    rgb = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    calib = cloud.read_calib_file(CALIB)
    vc = utils.voxel_down_sample(rgb, disp, calib, 0.02, depth_trunc=50.0)
    c = _calib()
    o = voxel_oracle.voxelize(disp, disp, disp, np.ascontiguousarray(rgb.transpose(2, 0, 1)), voxel_size=0.02, fx=c["fx"] / 2.0, fy=c["fx"] / 2.0,
                              cx=c["cx"] / 2.0, cy=c["cy"] / 2.0, baseline=c["baseline"], doffs=c["doffs"], depth_trunc=50.0, filtered=False)
    assert isinstance(vc, cloud.VoxelCloud) and vc.records.is_cuda and 20 < o["stats"][3] < o["stats"][0]
    _compare(vc, [o], tag=" utils")
    assert np.array_equal(vc.points(0).cpu().numpy().view(np.int32), o["records"][:, :3])
    assert np.array_equal(vc.weights(0).cpu().numpy(), o["weights"]) and vc.complete(0)


@functools.lru_cache(maxsize=1)
def _s_model():
    from s2m2_amd.model import S2M2
    from s2m2_amd.spec import MODEL_CONFIGS
    from s2m2_amd.weights import seeded_state_dict
    C, ntr = MODEL_CONFIGS["S"]
    m = S2M2(C, 1, ntr, use_positivity=True, refine_iter=3)
    m.load_state_dict(seeded_state_dict(C, 1, ntr, 0), strict=True)
    return m.cuda().eval()


def test_runner_writes_the_voxel_cloud(hip, tmp_path):
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
    out = tmp_path / "out"
    out.mkdir()
    common = ["--calib", CALIB, "--depth-trunc", "3", "--conf-min", "0.02"]
    p = subprocess.run([RUNNER, path, str(tmp_path / "left.f32"), str(tmp_path / "right.f32"), "--out", str(out)] + common +
                       ["--voxel", "0.05", "--voxel-ply", str(tmp_path / "v.ply"), "--ply", str(tmp_path / "full.ply"), "--repeat", "2"],
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr
    assert "voxel_us_per_pair" in p.stdout and "cloud_us_per_pair" in p.stdout
    maps = [torch.from_numpy(np.fromfile(out / f"{n}.f32", dtype="<f4").reshape(1, 1, H, W)).cuda() for n in ("disp", "occ", "conf")]
    kw = dict(depth_trunc=3.0, conf_min=0.02, **_calib())
    vc = cloud.voxelize(*maps, left.cuda(), voxel_size=0.05, **kw)
    pc = cloud.reproject(*maps, left.cuda(), **kw)
    torch.cuda.synchronize()
    print(f"[voxel runner] stats {vc.stats[0].tolist()}")
    assert vc.complete(0) and 0 < vc.size(0) < pc.size(0)
    assert cloud.read_ply_records(str(tmp_path / "v.ply")).tobytes() == vc.records[0, :vc.size(0)].cpu().numpy().tobytes()
    assert cloud.read_ply_records(str(tmp_path / "full.ply")).tobytes() == pc.records[0, :pc.size(0)].cpu().numpy().tobytes()
