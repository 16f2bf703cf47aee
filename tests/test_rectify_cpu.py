"""CPU-side checks of the rectifier (K16: include/s2m2_hip.h s2m2_rectify, s2m2_amd/rectify.py): properties that pin the host algorithm
without OpenCV, the glue functions, the boundary (symbols, descriptor layout, every validation path -- all return before any device call) and
the CEM search with an injected scorer."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rectify_oracle as O
from s2m2_amd import hip, rectify, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XML = os.path.join(ROOT, "tests", "golden", "calib_head.xml")
SIZE = (2048, 1536)


def _deltas():
    rng = np.random.RandomState(16)
    return [(0.0, 0.0, 0.0)] + [tuple(d) for d in rng.normal(0.0, 0.002, (4, 3))] + [(0.006, -0.006, 0.006)]


DELTAS = _deltas()
IDS = [f"delta{i}" for i in range(len(DELTAS))]


@pytest.fixture(scope="module")
def calib():
    return rectify.parse_xml_calibration(XML)


@pytest.fixture(scope="module")
def lib():
    from s2m2_amd.build import build
    build(verbose=False)
    return hip.load()


def _rect(calib, delta, size=SIZE):
    return rectify.compute_stereo_rectification(calib, size, rectify.create_delta_rotation(*delta))


# ------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("delta", DELTAS, ids=IDS)
def test_rotations_and_projections(calib, delta):
    r = _rect(calib, delta)
    for k in ("R1", "R2"):
        assert np.abs(r[k] @ r[k].T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(r[k]) - 1.0) < 1e-12
    assert np.abs(r["R2"] @ r["R"] @ r["R1"].T - np.eye(3)).max() < 1e-12
    t = r["R2"] @ r["T"]
    assert abs(t[1]) < 1e-12 * abs(t[0]) and abs(t[2]) < 1e-12 * abs(t[0])
    assert np.array_equal(r["P1"][:, :3], r["P2"][:, :3])
    assert abs(r["P2"][0, 3] - r["P1"][0, 0] * t[0]) <= 1e-12 * abs(r["P2"][0, 3])
    assert r["P1"][0, 3] == 0 and r["P2"][1, 3] == 0 and r["P1"][0, 0] == r["P1"][1, 1]
    assert all(r[k].dtype == np.float64 for k in ("K1", "D1", "K2", "D2", "R", "T", "R1", "R2", "P1", "P2", "Q"))
    assert not any(k in r for k in rectify.MAP_KEYS)


@pytest.mark.parametrize("delta", DELTAS, ids=IDS)
def test_epipolar_property(calib, delta):
    """Seeded 3-D points projected through the DISTORTED raw camera models into both raw images, then carried through the inverse map
    (undistort, R_k, P_k), land on equal rows, and their column difference is -P2[0][3] / Z_rect.
    Measured once over the six corrections (2000 points each, float64, undistortion converged to a residual below 4e-16 in normalised
    coordinates): row difference 5.7e-12 px, column-difference error 5.0e-12 px at most.  Asserted: 10 x the larger, 5.7e-11 px."""
    r = _rect(calib, delta)
    rng = np.random.RandomState(5)
    n = 2000
    Z = rng.uniform(0.5, 20.0, n)
    X1 = np.stack([rng.uniform(-0.55, 0.55, n) * Z, rng.uniform(-0.4, 0.4, n) * Z, Z])            # in the left camera's frame
    X2 = r["R"] @ X1 + r["T"][:, None]
    uv = []
    for X, K, D, Rk, P in ((X1, r["K1"], r["D1"], r["R1"], r["P1"]), (X2, r["K2"], r["D2"], r["R2"], r["P2"])):
        xd, yd = O.distort(X[0] / X[2], X[1] / X[2], D)
        raw = np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], axis=1)
        uv.append(O.undistort_points(raw, K, D, R=Rk, P=P))
    z_rect = (r["R1"] @ X1)[2]
    rows = np.abs(uv[0][:, 1] - uv[1][:, 1]).max()
    cols = np.abs((uv[0][:, 0] - uv[1][:, 0]) - (-r["P2"][0, 3] / z_rect)).max()
    print(f"epipolar: rows {rows:.3e} px, columns {cols:.3e} px")
    assert rows < 5.7e-11 and cols < 5.7e-11


@pytest.mark.parametrize("delta", DELTAS, ids=IDS)
def test_alpha_zero_crops_every_invalid_pixel_and_is_tight(calib, delta):
    r = _rect(calib, delta)
    W, H = SIZE
    slack = []
    for rec in rectify.rectification_records(r):
        mx, my = O.maps(rec, H, W)
        outside = (mx < 0) | (mx > W - 1) | (my < 0) | (my > H - 1)
        assert outside.mean() == 0.0
        slack += [mx.min(), W - 1 - mx.max(), my.min(), H - 1 - my.max()]
    print(f"alpha = 0: closest side of a map's bounding box {min(slack):.3f} px from the source border")
    assert 0.0 <= min(slack) < 3.0


def test_identity_rig():
    fx, cx, cy, W, H = 900.0, 400.0, 250.0, 832, 512
    cam = {"fx": fx, "fy": fx, "cx": cx, "cy": cy, "distortion": np.zeros(5)}
    c = {"left": dict(cam), "right": dict(cam), "stereo_extrinsic": {"rotation": np.eye(3), "translation": np.array([-0.12, 0.0, 0.0])}}
    r = rectify.compute_stereo_rectification(c, (W, H))
    assert np.abs(r["R1"] - np.eye(3)).max() < 1e-15 and np.abs(r["R2"] - np.eye(3)).max() < 1e-15
    f = r["P1"][0, 0]
    m = min(cx, cy, W - 1 - cx, H - 1 - cy)
    assert 1.0 <= f / fx <= 1.0 + 2.0 / m
    pcx, pcy = r["P1"][0, 2], r["P1"][1, 2]
    for rec in rectify.rectification_records(r):
        mx, my = O.maps(rec, H, W)
        u, v = np.arange(W)[None, :], np.arange(H)[:, None]
        assert np.abs(mx - (cx + (u - pcx) * fx / f)).max() < 1e-9 and np.abs(my - (cy + (v - pcy) * fx / f)).max() < 1e-9


@pytest.mark.parametrize("delta", DELTAS, ids=IDS)
def test_product_agrees_with_the_oracle(calib, delta):
    got = _rect(calib, delta)
    want = O.stereo_rectify(O.parse_xml(XML), SIZE, O.euler_xyz(*delta))
    for k, w in want.items():
        assert np.abs(got[k] - w).max() <= 1e-9 * np.abs(w).max(), k
    recs = rectify.rectification_records(got)
    for i, (K, D, Rk, P) in enumerate((("K1", "D1", "R1", "P1"), ("K2", "D2", "R2", "P2"))):
        w = O.make_record(i, want[K], want[D], want[Rk], want[P])
        assert np.abs(recs[i, :19] - w).max() <= 1e-9 * np.abs(w).max() and recs[i, 19] == 0


def test_window_camera_is_exact(calib):
    """the fixture windows: a camera with cx -= x0, cy -= y0 maps window pixel (u, v) where the full camera maps (u, v), minus the offset"""
    r = _rect(calib, (0.0, 0.0, 0.0))
    full = rectify.rectification_records(r)[0]
    win = full.copy()
    win[hip.RECTIFY_REC_FX + 2] -= 720
    win[hip.RECTIFY_REC_FX + 3] -= 560
    a, b = O.maps(full, 64, 64), O.maps(win, 64, 64)
    assert np.abs(a[0] - 720 - b[0]).max() < 1e-9 and np.abs(a[1] - 560 - b[1]).max() < 1e-9


def test_recorded_prototype_values(calib):
    """The drift guard: the float64 prototype of this algorithm recorded f = 1222.886, c = (1026.40, 757.26), P2[0][3] = -159.126 for this file
    at 2048 x 1536 without a correction.  The figures depend on when the fixed-point undistortion of the corner and grid points stops: run to
    a largest step below 1e-5 (30 steps here) it gives 1222.8864, (1026.3972, 757.2562), -159.1262; run to rounding level it gives
    1222.8927, (1026.4032, 757.2522), -159.12706, which is outside the digits recorded."""
    r = _rect(calib, (0.0, 0.0, 0.0))
    print(f"f = {r['P1'][0, 0]:.4f}  c = ({r['P1'][0, 2]:.4f}, {r['P1'][1, 2]:.4f})  P2[0][3] = {r['P2'][0, 3]:.5f}")
    assert abs(r["P1"][0, 2] - 1026.40) < 0.005
    assert abs(r["P1"][0, 0] - 1222.886) < 0.0005
    assert abs(r["P1"][1, 2] - 757.26) < 0.005
    assert abs(r["P2"][0, 3] - -159.126) < 0.0005


# ------------------------------------------------------------------------------------------------ glue
def test_euler_against_scipy():
    Rot = pytest.importorskip("scipy.spatial.transform").Rotation
    rng = np.random.RandomState(1)
    for a in list(rng.uniform(-3.0, 3.0, (20, 3))) + [np.zeros(3), np.array([0.006, -0.006, 0.006])]:
        assert np.abs(rectify.euler_to_rotation_matrix(*a) - Rot.from_euler("xyz", a).as_matrix()).max() < 1e-15
        assert np.array_equal(rectify.create_delta_rotation(*a), rectify.euler_to_rotation_matrix(*a))
    A, B = rectify.euler_to_rotation_matrix(0.1, 0.2, 0.3), rectify.euler_to_rotation_matrix(-0.3, 0.1, 0.2)
    assert np.array_equal(rectify.apply_delta_rotation(A, B), A @ B)
    assert rectify.build_camera_matrix(1.0, 2.0, 3.0, 4.0).tolist() == [[1, 0, 3], [0, 2, 4], [0, 0, 1]]


def test_xml_parser_on_the_fixture(calib, capsys):
    assert set(calib) == {"left", "right", "rgb", "stereo_extrinsic", "left2rgb"}
    assert calib["left"]["fx"] == 1308.1149274297488 and calib["left"]["cy"] == 759.9714992866387
    assert calib["right"]["fy"] == 1311.7861136252282 and calib["right"]["cx"] == 1027.6147469316727
    assert calib["left"]["distortion"].tolist() == [-0.22551825674840756, 0.1385294270787973, -0.0004237654817720754, 0.00028277921049612176,
                                                    -0.047782153963237234]
    assert calib["right"]["distortion"][4] == -0.05291040040948055 and calib["rgb"]["fx"] == calib["left"]["fx"]
    R, T = calib["stereo_extrinsic"]["rotation"], calib["stereo_extrinsic"]["translation"]
    assert R.shape == (3, 3) and R[0, 1] == -0.002483087412881868 and R[2, 2] == 0.999997308322102
    assert T.tolist() == [-0.1301186340535922, -0.00025794283659553237, -0.0010933857452932244]
    assert np.array_equal(calib["left2rgb"]["rotation"], np.eye(3)) and calib["left2rgb"]["translation"].tolist() == [0.0, 0.0, 0.0]
    loaded = rectify.load_calibration_data(XML)
    assert "Calibration data loaded" in capsys.readouterr().out and loaded["left"]["fx"] == calib["left"]["fx"]
    assert rectify.load_calibration_data(os.path.join(ROOT, "no_such.xml")) is None
    assert "XML calibration file not found" in capsys.readouterr().out
    assert rectify.load_calibration_data(os.path.join(ROOT, "README.md")) is None
    assert "Error loading calibration data" in capsys.readouterr().out


def test_structure_of_q(calib):
    r = _rect(calib, (0.001, -0.002, 0.0005))
    Q, f, cx, cy = r["Q"], r["P1"][0, 0], r["P1"][0, 2], r["P1"][1, 2]
    tx = r["P2"][0, 3] / f
    want = np.array([[1, 0, 0, -cx], [0, 1, 0, -cy], [0, 0, 0, f], [0, 0, -1.0 / tx, 0]])
    assert np.abs(Q - want).max() <= 1e-12 * np.abs(want).max()
    # a pixel with disparity d reprojects to depth f * |Tx| / d
    d = 25.0
    p = Q @ np.array([cx + 10, cy - 5, d, 1.0])
    assert abs(p[2] / p[3] - f * abs(tx) / d) < 1e-9


def test_reexports_in_utils():
    for name in ("parse_xml_calibration", "load_calibration_data", "euler_to_rotation_matrix", "create_delta_rotation", "apply_delta_rotation",
                 "build_camera_matrix", "compute_stereo_rectification", "rectify_images", "rectify_population", "evaluate_sample", "cem_calibration"):
        assert getattr(utils, name) is getattr(rectify, name)


# ------------------------------------------------------------------------------------------------ boundary
def _desc(**over):
    """a descriptor that passes validation (the pointers are never dereferenced on the host)"""
    d = hip.RectifyDesc()
    d.src[0], d.src[1] = 4096, 8192
    d.records, d.out, d.maps = 4096, 4096, 4096
    d.n_src, d.n_img, d.Hs, d.Ws, d.Hd, d.Wd, d.src_format, d.out_dtype, d.round, d.order = 2, 4, 48, 64, 48, 64, 0, 0, 1, 0
    for k, v in over.items():
        if k in ("src0", "src1"):
            d.src[int(k[3])] = v
        else:
            setattr(d, k, v)
    return d


def test_symbols_version_and_header_constants(lib):
    assert hasattr(lib, "s2m2_rectify") and "s2m2_rectify" in hip.SIGNATURES
    assert lib.s2m2_version() == 800 and hip.ABI_VERSION == 800
    header = open(os.path.join(ROOT, "include", "s2m2_hip.h")).read()
    assert int(re.search(r"#define S2M2_ABI_VERSION (\d+)", header).group(1)) == 800
    const = {k: int(v) for k, v in re.findall(r"(S2M2_RECTIFY_[A-Z0-9_]+) = (\d+)", header)}
    assert const["S2M2_RECTIFY_RECORD_FLOATS"] == hip.RECTIFY_RECORD_FLOATS == 20
    assert (const["S2M2_RECTIFY_REC_SRC"], const["S2M2_RECTIFY_REC_IR"], const["S2M2_RECTIFY_REC_FX"], const["S2M2_RECTIFY_REC_K1"]) == \
        (hip.RECTIFY_REC_SRC, hip.RECTIFY_REC_IR, hip.RECTIFY_REC_FX, hip.RECTIFY_REC_K1)
    assert [const[f"S2M2_RECTIFY_REC_{n}"] for n in ("FX", "FY", "CX", "CY", "K1", "K2", "P1", "P2", "K3")] == list(range(10, 19))
    assert (const["S2M2_RECTIFY_SRC_U8_HWC"], const["S2M2_RECTIFY_SRC_U8_CHW"], const["S2M2_RECTIFY_SRC_F32_CHW"]) == \
        (hip.RECTIFY_SRC_U8_HWC, hip.RECTIFY_SRC_U8_CHW, hip.RECTIFY_SRC_F32_CHW)
    assert (const["S2M2_RECTIFY_ORDER_SAMPLE"], const["S2M2_RECTIFY_ORDER_TILE"]) == (hip.RECTIFY_ORDER_SAMPLE, hip.RECTIFY_ORDER_TILE)
    assert "s2m2_rectify is NOT recorded" in header


def test_stale_library_without_the_symbol_asks_for_a_rebuild(lib, monkeypatch):
    class Stale:
        def __getattr__(self, name):
            if name == "s2m2_rectify":
                raise AttributeError(name)
            return getattr(lib, name)
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: Stale())
    with pytest.raises(RuntimeError, match="s2m2_rectify.*rebuild the library"):
        hip.load()


def test_rectify_desc_has_the_layout_of_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = [f[0] for f in hip.RectifyDesc._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "s2m2_hip.h"', "int main(void) {", "  s2m2_rectify_desc d;",
             '  printf("%zu\\n", sizeof(d));']
    lines += [f'  printf("{n} %zu %zu\\n", offsetof(s2m2_rectify_desc, {n}), sizeof(d.{n}));' for n in names]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == ctypes.sizeof(hip.RectifyDesc)
    for n, line in zip(names, out[1:]):
        name, off, size = line.split()
        f = getattr(hip.RectifyDesc, n)
        assert (name, int(off), int(size)) == (n, f.offset, f.size)


BAD = [
    (dict(records=None), b"null pointer (records)"),
    (dict(out=None, maps=None), b"no output requested"),
    (dict(src0=None), b"null pointer (src[0])"),
    (dict(src1=None), b"null pointer (src[1])"),
    (dict(n_src=0), b"n_src must be 1 or 2"),
    (dict(n_src=3), b"n_src must be 1 or 2"),
    (dict(n_img=0), b"non-positive extents"),
    (dict(Hs=0), b"non-positive extents"),
    (dict(Ws=-1), b"non-positive extents"),
    (dict(Hd=0), b"non-positive extents"),
    (dict(Wd=0), b"non-positive extents"),
    (dict(Hs=1 << 16, Ws=1 << 16), b"extents too large"),
    (dict(Wd=1 << 23), b"extents too large"),
    (dict(src_format=3), b"unsupported source format"),
    (dict(src_format=-1), b"unsupported source format"),
    (dict(out_dtype=1), b"unsupported output dtype"),
    (dict(out_dtype=3), b"unsupported output dtype"),
    (dict(order=2), b"unknown block order"),
    (dict(out=4098), b"fp32 output must be 4-byte aligned"),
    (dict(src_format=2, src0=4097), b"fp32 source must be 4-byte aligned"),
    (dict(records=4098), b"records and maps must be 4-byte aligned"),
    (dict(maps=4097), b"records and maps must be 4-byte aligned"),
    (dict(n_img=1 << 24, Hd=1 << 12, Wd=1 << 14), b"too many blocks"),
]


@pytest.mark.parametrize("over,msg", BAD, ids=[f"{'-'.join(o)}-{i}" for i, (o, _) in enumerate(BAD)])
def test_validation_fails_before_any_device_call(lib, over, msg):
    assert lib.s2m2_rectify(ctypes.byref(_desc(**over)), None) != 0
    assert msg in lib.s2m2_last_error(), lib.s2m2_last_error()


def test_null_descriptor(lib):
    assert lib.s2m2_rectify(None, None) != 0 and b"null descriptor" in lib.s2m2_last_error()


def test_refused_while_a_plan_records(lib):
    plan = ctypes.c_void_p()
    assert lib.s2m2_plan_begin(ctypes.byref(plan)) == 0
    try:
        assert lib.s2m2_rectify(ctypes.byref(_desc()), None) != 0
        assert b"not recorded in launch plans" in lib.s2m2_last_error()
        assert lib.s2m2_plan_launches(plan) == 0
    finally:
        lib.s2m2_plan_abort(plan)
        lib.s2m2_plan_destroy(plan)


def test_binding_rejects_host_tensors(calib):
    import torch
    img = torch.zeros(48, 64, 3, dtype=torch.uint8)
    rec = torch.zeros(2, hip.RECTIFY_RECORD_FLOATS)
    with pytest.raises(ValueError, match="device tensors"):
        hip.rectify([img, img], rec, torch.zeros(2, 3, 48, 64))
    with pytest.raises(ValueError, match="device tensors"):
        rectify.rectify_images(img, img, _rect(calib, (0.0, 0.0, 0.0), (64, 48)))
    with pytest.raises(ValueError, match="device tensors"):
        rectify.rectify_population(img, img, calib, [[0.0, 0.0, 0.0]])


# ------------------------------------------------------------------------------------------------ CEM with an injected scorer
HIDDEN = np.array([0.003, -0.002, 0.001])


def _peak(height):
    return lambda s: (height * np.exp(-((np.asarray(s) - HIDDEN) ** 2).sum(axis=1) / (2 * 0.003 ** 2))).tolist()


def test_cem_follows_the_reference_with_an_injected_scorer(calib, capsys):
    np.random.seed(0)
    first = np.random.normal(0, 0.002, (20, 3))
    np.random.seed(0)
    res = rectify.cem_calibration(None, None, None, calib, None, scorer=_peak(0.9))
    out = capsys.readouterr().out
    assert set(res) >= {"roll_delta", "pitch_delta", "yaw_delta", "initial_confidence", "final_confidence", "calib_data_new"}
    it = res["iterations"]
    assert len(it) == 5 and it[0]["samples"].shape == (21, 3) and it[0]["scores"].shape == (21,)
    assert np.array_equal(it[0]["samples"][0], np.zeros(3)) and np.array_equal(it[0]["samples"][1:], first)
    assert res["initial_confidence"] == it[0]["scores"][0] == _peak(0.9)(np.zeros((1, 3)))[0]
    # the elite update, the std decay and the floor, replayed from the recorded populations
    np.random.seed(0)
    mean, std, best = np.zeros(3), np.full(3, 0.002), res["initial_confidence"]
    bests = [best]
    for k in range(5):
        draw = np.random.normal(mean, std, (20, 3))
        assert np.array_equal(draw, it[k]["samples"][1:]) and np.array_equal(it[k]["samples"][0], mean)
        order = sorted(range(21), key=lambda i: it[k]["scores"][i], reverse=True)[:3]
        elite = it[k]["samples"][order]
        mean, std = elite.mean(axis=0), np.maximum(elite.std(axis=0) * 0.8, 0.00005)
        best = max(best, it[k]["scores"][order[0]])
        bests.append(best)
    assert bests == sorted(bests) and res["final_confidence"] == best and res["final_confidence"] >= res["initial_confidence"]
    assert np.all(std >= 0.00005)
    found = np.array([res["roll_delta"], res["pitch_delta"], res["yaw_delta"]])
    assert np.abs(found - HIDDEN).max() < 2e-4
    want = calib["stereo_extrinsic"]["rotation"] @ rectify.euler_to_rotation_matrix(*found)
    assert np.array_equal(res["calib_data_new"]["stereo_extrinsic"]["rotation"], want)
    assert res["calib_data_new"]["left"]["fx"] == calib["left"]["fx"] and res["calib_data_new"] is not calib
    for line in ("Starting CEM based online stereo calibration", "Iteration 1/5", "Iteration 5/5", "CEM CALIBRATION RESULTS", "Final deltas - Roll:"):
        assert line in out


def test_cem_std_floor_and_early_exit(calib, capsys):
    # a constant score: the elite are the mean and the first samples, the std collapses towards the floor of 5e-5 and never below it
    np.random.seed(1)
    res = rectify.cem_calibration(None, None, None, calib, None, scorer=lambda s: [0.5] * len(s), max_iterations=3, num_samples=5, num_elite=1)
    assert len(res["iterations"]) == 3 and res["final_confidence"] == 0.5
    np.random.seed(1)
    np.random.normal(np.zeros(3), np.full(3, 0.002), (5, 3))
    second = np.random.normal(np.zeros(3), np.full(3, 0.00005), (5, 3))            # one elite: std 0 * decay -> the floor
    assert np.array_equal(res["iterations"][1]["samples"][1:], second)
    # early exit: above 0.98 before the first iteration, and after the first one
    res = rectify.cem_calibration(None, None, None, calib, None, scorer=lambda s: [0.99] * len(s))
    assert res["iterations"] == [] and res["final_confidence"] == 0.99 and res["roll_delta"] == 0.0
    assert "Iteration 1/" not in capsys.readouterr().out.split("Starting CEM")[-1]
    np.random.seed(2)
    res = rectify.cem_calibration(None, None, None, calib, None, scorer=lambda s: [0.5 if not np.any(s[i]) else 0.985 for i in range(len(s))])
    assert len(res["iterations"]) == 1 and res["final_confidence"] == 0.985
    # num_elite above num_samples is clamped with the reference's warning
    rectify.cem_calibration(None, None, None, calib, None, scorer=lambda s: [0.1] * len(s), max_iterations=1, num_samples=2, num_elite=5)
    assert "Setting num_elite to num_samples" in capsys.readouterr().out
