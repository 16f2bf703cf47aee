"""GPU tests of the rectifier (K16, s2m2_rectify) against the float64 numpy oracle in tests/rectify_oracle.py.

Tolerances are measured, not chosen: E32 is the largest deviation of the oracle's map formula evaluated in numpy float32 (from the same fp32
record) from its float64 evaluation; the kernel's maps may deviate by 4 x E32 (another operation order, fused multiply-adds).  Every figure is
printed before it is asserted; with S2M2_RECTIFY_PARITY_OUT=<file> the figures are appended to that file (profiles/rectify/parity.txt)."""
import os

import numpy as np
import pytest
import torch

import rectify_oracle as O
from s2m2_amd import hip, rectify
from s2m2_amd import utils as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
XML = os.path.join(GOLDEN, "calib_head.xml")
NF = hip.RECTIFY_RECORD_FLOATS


def _note(line):
    print(line)
    path = os.environ.get("S2M2_RECTIFY_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _deltas():
    rng = np.random.RandomState(16)
    return [(0.0, 0.0, 0.0)] + [tuple(d) for d in rng.normal(0.0, 0.002, (2, 3))] + [(0.006, -0.006, 0.006)]


@pytest.fixture(scope="module")
def calib():
    return rectify.parse_xml_calibration(XML)


@pytest.fixture(scope="module")
def window():
    l, r = (np.load(os.path.join(GOLDEN, f"rectify_raw_{s}_window.npz")) for s in ("left", "right"))
    assert l["offset"].tolist() == r["offset"].tolist()
    return l["image"], r["image"], int(l["offset"][0]), int(l["offset"][1])


def _rec32(rec64):
    """(n, NF) float64 -> what the device holds"""
    out = np.zeros((len(rec64), NF), dtype=np.float32)
    out[:, :rec64.shape[1]] = rec64
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(srcs, rec32, Hd, Wd, dtype=torch.float32, round=True, maps=False, order=hip.RECTIFY_ORDER_SAMPLE):
    out = torch.empty((len(rec32), 3, Hd, Wd), device="cuda", dtype=dtype)
    mp = torch.empty((len(rec32), 2, Hd, Wd), device="cuda", dtype=torch.float32) if maps else None
    hip.rectify([_dev(s) if isinstance(s, np.ndarray) else s for s in srcs], _dev(rec32), out, mp, round=round, order=order)
    torch.cuda.synchronize()
    return (out.cpu().numpy(), mp.cpu().numpy()) if maps else out.cpu().numpy()


def _synthetic_record(W, H, src=0):
    """a strongly distorted camera under a small rotation and a new projection, written by hand"""
    K = np.array([[0.62 * W, 0, 0.52 * W], [0, 0.63 * W, 0.47 * H], [0, 0, 1.0]])
    D = np.array([-0.31, 0.12, 0.002, -0.003, -0.02])
    Rk = O.rot(np.array([0.02, -0.03, 0.015]))
    P = np.array([[0.8 * W, 0, 0.5 * W, 0], [0, 0.8 * W, 0.5 * H, 0], [0, 0, 1.0, 0]])
    return O.make_record(src, K, D, Rk, P)


def _e32(rec32, Hd, Wd):
    m64 = O.maps(rec32.astype(np.float64), Hd, Wd)
    m32 = O.maps(rec32, Hd, Wd, np.float32)
    return max(np.abs(m32[0] - m64[0]).max(), np.abs(m32[1] - m64[1]).max()), m64


def _analytic(H, W, seed):
    """sum of sinusoids in [0,255] with a known Lipschitz constant (levels per pixel, both directions)"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.full((3, H, W), 127.5)
    L = 0.0
    for c in range(3):
        Lc = 0.0
        for _ in range(4):
            a, wx, wy, ph = rng.uniform(5, 30), rng.uniform(0.02, 0.5), rng.uniform(0.02, 0.5), rng.uniform(0, 6.28)
            img[c] += a * np.sin(wx * x + wy * y + ph)
            Lc += a * max(wx, wy)                       # |d/dx| <= a wx and |d/dy| <= a wy
        L = max(L, Lc)
    assert img.min() >= 0 and img.max() <= 255
    return img.astype(np.float32), L


# ------------------------------------------------------------------------------------------------ maps
def test_maps_against_the_float64_oracle_full_size(calib):
    W, H = 2048, 1536
    dummy = torch.zeros((3, H, W), device="cuda", dtype=torch.uint8)
    for delta in _deltas():
        r = rectify.compute_stereo_rectification(calib, (W, H), rectify.create_delta_rotation(*delta))
        rec = _rec32(rectify.rectification_records(r))
        mp = torch.empty((2, 2, H, W), device="cuda", dtype=torch.float32)
        hip.rectify([dummy], _dev(rec), None, mp)
        got = mp.cpu().numpy().astype(np.float64)
        for cam in range(2):
            e32, m64 = _e32(rec[cam], H, W)
            err = max(np.abs(got[cam, 0] - m64[0]).max(), np.abs(got[cam, 1] - m64[1]).max())
            _note(f"maps 2048x1536 delta {tuple(round(float(d), 5) for d in delta)} camera {cam}: E32 {e32:.3e} px, kernel {err:.3e} px (bound {4 * e32:.3e})")
            assert err <= 4 * e32
    # want_maps: the kernel's maps under the reference's keys
    r = rectify.compute_stereo_rectification(calib, (W, H), want_maps=True)
    assert all(r[k].is_cuda and tuple(r[k].shape) == (H, W) and r[k].dtype == torch.float32 for k in rectify.MAP_KEYS)
    rec0 = _rec32(rectify.rectification_records(r))
    e32, m64 = _e32(rec0[0], H, W)
    assert np.abs(r["leftMapX"].cpu().numpy() - m64[0]).max() <= 4 * e32


def test_maps_strongly_distorted_synthetic_camera():
    W, H = 803, 601
    rec = _rec32(np.stack([_synthetic_record(W, H)]))
    _, mp = _run([np.zeros((H, W, 3), np.uint8)], rec, H, W, maps=True)
    e32, m64 = _e32(rec[0], H, W)
    err = max(np.abs(mp[0, 0] - m64[0]).max(), np.abs(mp[0, 1] - m64[1]).max())
    _note(f"maps 803x601 synthetic k1 = -0.31: E32 {e32:.3e} px, kernel {err:.3e} px (bound {4 * e32:.3e})")
    assert err <= 4 * e32


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("case", ["fixture", "synthetic"])
def test_unrounded_values_on_analytic_images(calib, case):
    """every pixel: |out - oracle| <= L (|dmapx| + |dmapy|) + 255 * 2^-21 with |dmap| <= 4 E32 each"""
    W, H = (640, 480) if case == "fixture" else (803, 601)
    if case == "fixture":
        c = O.window_calib(calib, 700, 500)
        rec = _rec32(rectify.rectification_records(rectify.compute_stereo_rectification(c, (W, H), rectify.create_delta_rotation(0.004, -0.002, 0.003))))
    else:
        rec = _rec32(np.stack([_synthetic_record(W, H, 0), _synthetic_record(W, H, 1)]))
    a, La = _analytic(H, W, 1)
    b, Lb = _analytic(H, W, 2)
    out = _run([a, b], rec, H, W, round=False)
    for i, (img, L) in enumerate(((a, La), (b, Lb))):
        e32, m64 = _e32(rec[i], H, W)
        want = O.remap(img, *m64)
        err = np.abs(out[i] - want).max()
        bound = L * 2 * 4 * e32 + 255 * 2.0 ** -21
        _note(f"values unrounded {case} image {i}: L {L:.2f} levels/px, E32 {e32:.3e} px, max error {err:.3e} (bound {bound:.3e})")
        assert err <= bound


def _rounded_check(name, srcs, rec, H, W):
    out = _run(srcs, rec, H, W, round=True)
    for i in range(len(rec)):
        img = srcs[int(rec[i, 0])].transpose(2, 0, 1)
        want64 = O.levels(O.rectify(img, rec[i].astype(np.float64), H, W))
        want32 = O.levels(O.rectify(img, rec[i], H, W, np.float32))
        diff = np.abs(out[i] - want64)
        share, share32 = float((diff != 0).mean()), float((want32 != want64).mean())
        _note(f"values rounded {name} record {i}: max |out - round(oracle)| {diff.max():.0f}, share differing {share:.3e} "
              f"(float32 numpy oracle {share32:.3e}, bound {2 * share32:.3e})")
        assert diff.max() <= 1
        assert share <= 2 * share32
    return out


def test_rounded_values_on_uint8_noise(calib):
    W, H = 640, 480
    rng = np.random.RandomState(3)
    srcs = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2)]
    c = O.window_calib(calib, 700, 500)
    rec = _rec32(rectify.population_records(c, (W, H), [(0.0, 0.0, 0.0), (0.003, -0.001, 0.002)]))
    _rounded_check("noise 640x480", srcs, rec, H, W)


def test_rounded_values_on_the_real_image_window(calib, window):
    left, right, x0, y0 = window
    H, W = left.shape[:2]
    rec = _rec32(rectify.population_records(O.window_calib(calib, x0, y0), (W, H), [(0.0, 0.0, 0.0), (-0.002, 0.001, 0.0015)]))
    out = _rounded_check("real window 608x416", [left, right], rec, H, W)
    # the public call gives the same pixels
    l, r = rectify.rectify_population(left, right, O.window_calib(calib, x0, y0), [(0.0, 0.0, 0.0), (-0.002, 0.001, 0.0015)])
    assert np.array_equal(l.cpu().numpy(), out[:2]) and np.array_equal(r.cpu().numpy(), out[2:])


def test_identity_record_returns_the_raw_image():
    W, H = 203, 97
    rng = np.random.RandomState(4)
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    rec = np.zeros((1, NF), dtype=np.float32)
    fx, fy, cx, cy = 256.0, 128.0, 64.0, 32.0                                   # powers of two: inv(K) is exact in fp32
    rec[0, 1:10] = [1 / fx, 0, -cx / fx, 0, 1 / fy, -cy / fy, 0, 0, 1]
    rec[0, 10:14] = fx, fy, cx, cy
    for dtype in (torch.float32, torch.uint8):
        out = _run([img], rec, H, W, dtype=dtype)
        assert np.array_equal(out[0], img.transpose(2, 0, 1))


def test_border_translation_and_magnification():
    """a translation by (-10.5, +7.25) px and a magnification past the source against the oracle's zero-border taps, half-covered footprints
    included (dyadic weights: the float64 oracle and the kernel are both exact, so unrounded outputs are equal)"""
    W, H = 150, 90
    rng = np.random.RandomState(6)
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    rec = np.zeros((2, NF), dtype=np.float32)
    rec[0, 1:10] = [1, 0, -10.5, 0, 1, 7.25, 0, 0, 1]                           # mapx = u - 10.5, mapy = v + 7.25
    rec[1, 1:10] = [2, 0, -100.5, 0, 2, -50.25, 0, 0, 1]                        # mapx = 2u - 100.5: leaves the source on every side
    rec[:, 10:14] = 1, 1, 0, 0
    out, mp = _run([img], rec, H, W, round=False, maps=True)
    for i in range(2):
        mx, my = O.maps(rec[i].astype(np.float64), H, W)
        assert np.array_equal(mp[i, 0], mx) and np.array_equal(mp[i, 1], my)
        want = O.remap(img.transpose(2, 0, 1), mx, my)
        assert np.array_equal(out[i].astype(np.float64), want)
    assert (out[0][:, :, :10] == 0).all() and (out[0][:, :, 10] != 0).any()    # column 10 is the half-covered one: mapx = -0.5
    assert (out[0][:, H - 7:, :] == 0).all() and (out[0][:, H - 8, 11:] != 0).any()   # row H-8: mapy = H - 0.75, three-quarter covered; H-7 is outside
    assert np.array_equal(out[0][:, 0, 11], 0.75 * (0.5 * img[7, 0] + 0.5 * img[7, 1]) + 0.25 * (0.5 * img[8, 0] + 0.5 * img[8, 1]))
    assert (out[1][:, :, :50] == 0).all() and (out[1][:, :25, :] == 0).all() and (out[1][:, :, 126:] == 0).all() and (out[1][:, 71:, :] == 0).all()
    rounded = _run([img], rec, H, W, round=True)
    assert np.array_equal(rounded, np.rint(out))
    nan = rec.copy()
    nan[0, 1:10] = [1, 0, 0, 0, 1, 0, 0, 0, 0]                                  # W = 0 everywhere: inf / NaN maps are all border
    assert (_run([img], nan[:1], H, W) == 0).all()


# ------------------------------------------------------------------------------------------------ population and interface
def test_population_single_calls_determinism_formats_and_sizes(calib):
    rng = np.random.RandomState(8)
    for (W, H), n_pairs in (((333, 205), 21), ((130, 66), 1), ((64, 48), 1), ((257, 9), 3)):
        srcs = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2)]
        c = O.window_calib(calib, 1024 - W // 2, 768 - H // 2)
        deltas = rng.normal(0, 0.002, (n_pairs, 3))
        rec = _rec32(rectify.population_records(c, (W, H), deltas))
        recs = {"all": rec, "one": rec[:1]} if n_pairs == 1 else {"all": rec}
        for name, rc in recs.items():                                           # n_img = 42, 2, 1, 6
            out = _run(srcs, rc, H, W)
            again = _run(srcs, rc, H, W)
            assert np.array_equal(out, again)
            singles = np.concatenate([_run(srcs, rc[i:i + 1], H, W) for i in range(len(rc))])
            assert np.array_equal(out, singles)
            assert np.array_equal(out, _run(srcs, rc, H, W, order=hip.RECTIFY_ORDER_TILE))
            u8 = _run(srcs, rc, H, W, dtype=torch.uint8)
            assert np.array_equal(u8.astype(np.float32), out)
            planar = [np.ascontiguousarray(s.transpose(2, 0, 1)) for s in srcs]
            assert np.array_equal(_run(planar, rc, H, W), out)
            assert np.array_equal(_run([p.astype(np.float32) for p in planar], rc, H, W), out)
            unrounded = _run(srcs, rc, H, W, round=False)
            assert np.array_equal(np.rint(unrounded), out) and not np.array_equal(unrounded, out)
            # one source only: records reading source 1 are clamped to the last source
            if name == "all":
                lone = rc.copy()
                lone[:, 0] = 0
                assert np.array_equal(_run(srcs[:1], rc, H, W), _run(srcs[:1], lone, H, W))


def test_graph_capture_and_replay_after_rewriting_the_records(calib, window):
    left, right, x0, y0 = window
    H, W = left.shape[:2]
    c = O.window_calib(calib, x0, y0)
    l, r = _dev(left), _dev(right)
    first = [(0.0, 0.0, 0.0), (0.001, 0.002, -0.001), (-0.003, 0.0, 0.002)]
    second = [(0.002, -0.002, 0.001), (0.0, 0.0015, 0.0), (0.004, 0.001, -0.002)]
    records = _dev(_rec32(rectify.population_records(c, (W, H), first)))
    out = torch.empty((6, 3, H, W), device="cuda", dtype=torch.uint8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.rectify([l, r], records, out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.rectify([l, r], records, out)
    for deltas in (first, second):
        records.copy_(_dev(_rec32(rectify.population_records(c, (W, H), deltas))))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        el, er = rectify.rectify_population(l, r, c, deltas, out_dtype=torch.uint8)
        assert torch.equal(out[:3], el) and torch.equal(out[3:], er)


def test_rectify_images_and_device_inputs(calib, window):
    left, right, x0, y0 = window
    H, W = left.shape[:2]
    c = O.window_calib(calib, x0, y0)
    data = rectify.compute_stereo_rectification(c, (W, H), rectify.create_delta_rotation(0.001, 0.0, -0.001))
    lr, rr = rectify.rectify_images(left, right, data)
    assert lr.is_cuda and lr.dtype == torch.uint8 and tuple(lr.shape) == (H, W, 3) and lr.permute(2, 0, 1).is_contiguous()
    l2, r2 = rectify.rectify_images(_dev(left), _dev(right), data)
    assert torch.equal(lr, l2) and torch.equal(rr, r2)
    pl, pr = rectify.rectify_population(left, right, c, [(0.001, 0.0, -0.001)], out_dtype=torch.uint8)
    assert torch.equal(pl[0], lr.permute(2, 0, 1)) and torch.equal(pr[0], rr.permute(2, 0, 1))
    assert pl.dtype == torch.uint8 and rectify.rectify_population(left, right, c, [(0.0, 0.0, 0.0)])[0].dtype == torch.float32


# ------------------------------------------------------------------------------------------------ end to end
def _model(ri=1):
    from s2m2_amd.model import S2M2
    from s2m2_amd.weights import seeded_state_dict
    m = S2M2(128, 1, 1, use_positivity=True, refine_iter=ri)
    m.load_state_dict(seeded_state_dict(128, 1, 1, 2), strict=True)
    return m.cuda().eval()


def test_cem_scores_equal_individually_rectified_pairs(calib, window, capsys):
    """random weights: the score carries no meaning, convergence is not asserted here (tests/test_rectify_cpu.py covers the search)"""
    left, right, x0, y0 = window
    c = O.window_calib(calib, x0, y0)
    m = _model()
    dev = torch.device("cuda")
    np.random.seed(11)
    res = rectify.cem_calibration(m, left, right, c, dev, max_iterations=1, num_samples=4)
    assert "Error evaluating sample" not in capsys.readouterr().out
    assert len(res["iterations"]) == 1
    if True:
        it = res["iterations"][0]
        assert it["scores"].shape == (5,) and np.isfinite(it["scores"]).all() and (it["scores"] > 0).all()
        for k in range(5):
            data = rectify.compute_stereo_rectification(c, (left.shape[1], left.shape[0]), rectify.create_delta_rotation(*it["samples"][k]))
            lr, rr = rectify.rectify_images(left, right, data)
            one = U.compute_confidence_score(m, lr.permute(2, 0, 1)[None], rr.permute(2, 0, 1)[None], dev)
            assert abs(one - it["scores"][k]) < 1e-5, (k, one, it["scores"][k])
        assert rectify.evaluate_sample(m, left, right, c, dev, 0.0, 0.0, 0.0) == pytest.approx(it["scores"][0], abs=1e-5)
    assert res["initial_confidence"] == pytest.approx(rectify.evaluate_sample(m, left, right, c, dev, 0, 0, 0), abs=1e-5)
    # the reference's contract for a failing evaluation
    assert rectify.evaluate_sample(m, left[:, :, :2], right, c, dev, 0, 0, 0) == 0.0
    assert "Error evaluating sample" in capsys.readouterr().out


def test_full_size_population_through_the_forward(calib):
    W, H = 2048, 1536
    rng = np.random.RandomState(9)
    base = rng.randint(0, 256, (H // 8, W // 8, 3)).astype(np.uint8)
    left = np.ascontiguousarray(np.kron(base, np.ones((8, 8, 1), dtype=np.uint8)))
    right = np.ascontiguousarray(np.roll(left, -16, axis=1))
    l, r = rectify.rectify_population(left, right, calib, [(0.0, 0.0, 0.0), (0.001, -0.001, 0.0005)])
    assert tuple(l.shape) == (2, 3, H, W) and l.dtype == torch.float32
    m = _model()
    with torch.autocast("cuda", dtype=torch.float16):
        disp, occ, conf = m(l, r)
    torch.cuda.synchronize()
    for t in (disp, occ, conf):
        assert tuple(t.shape[-2:]) == (H, W) and torch.isfinite(t).all()
