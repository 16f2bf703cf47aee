"""Rectification of raw stereo pairs on the device and CEM online calibration (K16, ``s2m2_rectify``) -- what sits in front of ``S2M2.forward``.

Counterparts of the reference's calibration glue with the same names, arguments and returned dict keys (src/s2m2/core/utils/calib_utils.py,
image_utils.py:108-136, calibration/base.py:15-36, calibration/cem.py), numpy only on the host: neither cv2 nor scipy is needed.

The split: the matrix work of a rectification -- Bouguet's algorithm as ``cv2.stereoRectify`` runs it for ``CALIB_ZERO_DISPARITY``,
``alpha = 0`` -- is a dozen 3x3 operations and 2 x 85 undistorted points, done here in float64.  The per-pixel work (the inverse map through the
distortion model and the bilinear gather, ``cv2.initUndistortRectifyMap`` + ``cv2.remap``) is one HIP launch for a whole population of
candidate rectifications; the raw pair is uploaded once.  The kernel interpolates at the full fp32 coordinate, where cv2.remap quantises to
1/32 px (include/s2m2_hip.h, K16).

Conventions where OpenCV versions differ: the image corners and the 9 x 9 grid of the alpha = 0 scaling span 0 .. nx-1 / 0 .. ny-1, the
border distances of that scaling are measured to nx, ny; point undistortion is OpenCV's fixed-point iteration run until the largest step over
the point set is below 1e-5 in normalised coordinates.
"""
from __future__ import annotations

import copy
import os
import xml.etree.ElementTree as ET
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np

MAP_KEYS = ("leftMapX", "leftMapY", "rightMapX", "rightMapY")


# ------------------------------------------------------------------------------------------------ calibration file
def _floats(text: str) -> np.ndarray:
    return np.array([float(x.strip()) for x in text.split(",")])


def parse_xml_calibration(calib_xml_path: str) -> Dict[str, dict]:
    """The rig's XML -> ``{'left','right','rgb': {fx, fy, cx, cy, distortion}, 'stereo_extrinsic','left2rgb': {rotation, translation}}``."""
    root = ET.parse(calib_xml_path).getroot()
    data: Dict[str, dict] = {}
    for key in ("left", "right", "rgb"):
        node = root.find(f"distorted_{key}_intrinsic")
        data[key] = {"fx": float(node.find("fx").text), "fy": float(node.find("fy").text), "cx": float(node.find("cx").text),
                     "cy": float(node.find("cy").text), "distortion": _floats(node.find("dist").text)}
    for key in ("stereo_extrinsic", "left2rgb"):
        node = root.find(key)
        data[key] = {"rotation": _floats(node.find("rotation").text).reshape(3, 3), "translation": _floats(node.find("translation").text)}
    return data


def load_calibration_data(calib_xml_path: str):
    """Same contract as the reference: the parsed dict, or None after printing why."""
    if not os.path.exists(calib_xml_path):
        print(f"XML calibration file not found: {calib_xml_path}")
        return None
    try:
        calib_data = parse_xml_calibration(calib_xml_path)
        print("Calibration data loaded")
        return calib_data
    except Exception as e:  # noqa: BLE001  (the reference swallows and reports)
        print(f"Error loading calibration data: {e}")
        return None


# ------------------------------------------------------------------------------------------------ rotations
def euler_to_rotation_matrix(roll: float, pitch: float, yaw: float) -> np.ndarray:
    """Extrinsic x-y-z Euler angles (radians) -> matrix, as ``scipy.spatial.transform.Rotation.from_euler('xyz', ...)``: Rz(yaw) Ry(pitch) Rx(roll)."""
    sx, cx, sy, cy, sz, cz = np.sin(roll), np.cos(roll), np.sin(pitch), np.cos(pitch), np.sin(yaw), np.cos(yaw)
    return np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                     [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                     [-sy, cy * sx, cy * cx]], dtype=np.float64)


def create_delta_rotation(roll_delta: float = 0.0, pitch_delta: float = 0.0, yaw_delta: float = 0.0) -> np.ndarray:
    return euler_to_rotation_matrix(roll_delta, pitch_delta, yaw_delta)


def apply_delta_rotation(original_R: np.ndarray, delta_R: np.ndarray) -> np.ndarray:
    return original_R @ delta_R


def build_camera_matrix(fx: float, fy: float, cx: float, cy: float) -> np.ndarray:
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float64)


def _skew(k: np.ndarray) -> np.ndarray:
    return np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])


def _rot(vec: np.ndarray) -> np.ndarray:
    """Rodrigues: rotation vector -> matrix"""
    theta = float(np.sqrt(vec @ vec))
    if theta == 0.0:
        return np.eye(3)
    S = _skew(vec / theta)
    return np.eye(3) + np.sin(theta) * S + (1.0 - np.cos(theta)) * (S @ S)


def _rotvec(R: np.ndarray) -> np.ndarray:
    """Rodrigues: matrix -> rotation vector (angle below pi); sine from the antisymmetric part, so small angles keep their precision"""
    axis = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sin_t = float(np.sqrt(axis @ axis))
    if sin_t == 0.0:
        return axis
    return axis * (np.arctan2(sin_t, 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0)) / sin_t)


# ------------------------------------------------------------------------------------------------ distortion model
UNDISTORT_TOL = 1e-5          # normalised coordinates; with at most UNDISTORT_MAX_ITER steps
UNDISTORT_MAX_ITER = 1000


def _undistort(xd: np.ndarray, yd: np.ndarray, D) -> Tuple[np.ndarray, np.ndarray]:
    """Normalised distorted -> undistorted coordinates of a point set: OpenCV's fixed-point iteration of the inverse model, iterated until it
    has converged -- the largest step over the set is below UNDISTORT_TOL -- instead of OpenCV's five times.  This is the termination rule of
    the float64 prototype whose figures tests/test_rectify_cpu.py records: the points only choose the new focal length and
    principal point, which are free parameters of a rectification, so the rule decides the crop and the centring by some thousandths of a
    pixel and nothing about the epipolar geometry."""
    k1, k2, p1, p2, k3 = D[:5]
    x, y = xd.astype(np.float64), yd.astype(np.float64)
    for _ in range(UNDISTORT_MAX_ITER):
        r2 = x * x + y * y
        inv = 1.0 / (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3)))
        xn, yn = (xd - (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))) * inv, (yd - (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)) * inv
        step = max(float(np.abs(xn - x).max()), float(np.abs(yn - y).max()))
        x, y = xn, yn
        if step < UNDISTORT_TOL:
            break
    return x, y


def _undistort_rotate_project(pts: np.ndarray, K: np.ndarray, D, R: np.ndarray, f: float, c=(0.0, 0.0)) -> np.ndarray:
    """raw pixel coordinates (n,2) -> undistorted, rotated by R, projected with focal length f and principal point c"""
    x, y = _undistort((pts[:, 0] - K[0, 2]) / K[0, 0], (pts[:, 1] - K[1, 2]) / K[1, 1], D)
    q = np.stack([x, y, np.ones_like(x)], axis=1) @ R.T
    return np.stack([f * q[:, 0] / q[:, 2] + c[0], f * q[:, 1] / q[:, 2] + c[1]], axis=1)


# ------------------------------------------------------------------------------------------------ stereoRectify
def compute_stereo_rectification(calibration_data: dict, image_size: Tuple[int, int], delta_R: Optional[np.ndarray] = None, *,
                                 want_maps: bool = False, device=None) -> Dict[str, object]:
    """``image_size`` = (width, height).  Returns K1, D1, K2, D2, R, T, R1, R2, P1, P2, Q as float64 arrays on the host: Bouguet's algorithm
    as ``cv2.stereoRectify(..., flags=CALIB_ZERO_DISPARITY, alpha=0)`` runs it, horizontal or vertical rig.  The four map arrays the reference
    also returns are what the kernel replaces, so they are not computed by default; ``want_maps=True`` has the kernel produce them and returns
    them as (H,W) fp32 device tensors (on ``device``, default the current one) under the reference's keys."""
    nx, ny = int(image_size[0]), int(image_size[1])
    left, right = calibration_data["left"], calibration_data["right"]
    Ks = (build_camera_matrix(left["fx"], left["fy"], left["cx"], left["cy"]), build_camera_matrix(right["fx"], right["fy"], right["cx"], right["cy"]))
    Ds = (np.asarray(left["distortion"], dtype=np.float64), np.asarray(right["distortion"], dtype=np.float64))
    R = np.asarray(calibration_data["stereo_extrinsic"]["rotation"], dtype=np.float64)
    T = np.asarray(calibration_data["stereo_extrinsic"]["translation"], dtype=np.float64).reshape(3)
    if delta_R is not None:
        R = R @ delta_R
    # each camera takes half of the rotation between them; then both are turned so that the baseline lies along the dominant image axis
    half = _rot(-0.5 * _rotvec(R))
    t = half @ T
    idx = 0 if abs(t[0]) > abs(t[1]) else 1
    e = np.zeros(3)
    e[idx] = 1.0 if t[idx] > 0 else -1.0
    w = np.cross(t, e)
    wn = float(np.sqrt(w @ w))
    if wn > 0.0:
        w *= np.arccos(abs(t[idx]) / float(np.sqrt(t @ t))) / wn
    turn = _rot(w)
    R1, R2 = turn @ half.T, turn @ half
    t = R2 @ T
    # new focal length: the smaller one across the cameras, shrunk for barrel distortion
    focal = []
    for K, D in zip(Ks, Ds):
        fc = K[idx ^ 1, idx ^ 1]
        focal.append(fc * (1.0 + D[0] * (nx * nx + ny * ny) / (4.0 * fc * fc)) if D[0] < 0 else fc)
    f = min(focal)
    # principal points: centre the rectified corners, then one point for both cameras (zero disparity)
    corners = np.array([[0.0, 0.0], [nx - 1.0, 0.0], [0.0, ny - 1.0], [nx - 1.0, ny - 1.0]])
    centre = np.array([(nx - 1) * 0.5, (ny - 1) * 0.5])
    c = 0.5 * sum(centre - _undistort_rotate_project(corners, K, D, Rk, f).mean(axis=0) for K, D, Rk in zip(Ks, Ds, (R1, R2)))
    # alpha = 0: scale the focal length until the inner rectangle of valid pixels fills the image
    steps = np.arange(9) / 8.0
    grid = np.stack([np.tile(steps * (nx - 1), 9), np.repeat(steps * (ny - 1), 9)], axis=1)
    s = 0.0
    for K, D, Rk in zip(Ks, Ds, (R1, R2)):
        g = _undistort_rotate_project(grid, K, D, Rk, f, c).reshape(9, 9, 2)           # [row, column]
        inner_x0, inner_x1 = g[:, 0, 0].max(), g[:, 8, 0].min()
        inner_y0, inner_y1 = g[0, :, 1].max(), g[8, :, 1].min()
        s = max(s, c[0] / (c[0] - inner_x0), c[1] / (c[1] - inner_y0), (nx - c[0]) / (inner_x1 - c[0]), (ny - c[1]) / (inner_y1 - c[1]))
    f *= s
    P1 = np.array([[f, 0.0, c[0], 0.0], [0.0, f, c[1], 0.0], [0.0, 0.0, 1.0, 0.0]])
    P2 = P1.copy()
    P2[idx, 3] = t[idx] * f
    Q = np.array([[1.0, 0.0, 0.0, -c[0]], [0.0, 1.0, 0.0, -c[1]], [0.0, 0.0, 0.0, f], [0.0, 0.0, -1.0 / t[idx], 0.0]])
    out: Dict[str, object] = {"K1": Ks[0], "D1": Ds[0], "K2": Ks[1], "D2": Ds[1], "R": R, "T": T, "R1": R1, "R2": R2, "P1": P1, "P2": P2, "Q": Q}
    if want_maps:
        import torch
        from . import hip
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        maps = torch.empty((2, 2, ny, nx), device=dev, dtype=torch.float32)
        extents = torch.empty((3, ny, nx), device=dev, dtype=torch.uint8)          # never read: without `out` a source only gives Hs, Ws
        hip.rectify([extents], _upload(rectification_records(out), dev), None, maps)
        out.update(zip(MAP_KEYS, (maps[0, 0], maps[0, 1], maps[1, 0], maps[1, 1])))
    return out


# ------------------------------------------------------------------------------------------------ records and launches
def camera_record(src: int, K: np.ndarray, D, R_rect: np.ndarray, P: np.ndarray) -> np.ndarray:
    """One K16 record (include/s2m2_hip.h: S2M2_RECTIFY_REC_*) in float64: source index, iR = inv(P[:, :3] R_rect), fx fy cx cy, k1 k2 p1 p2 k3."""
    from .hip import RECTIFY_RECORD_FLOATS, RECTIFY_REC_FX, RECTIFY_REC_IR, RECTIFY_REC_K1, RECTIFY_REC_SRC
    D = np.asarray(D, dtype=np.float64).reshape(-1)
    if D.size < 5:
        D = np.concatenate([D, np.zeros(5 - D.size)])
    rec = np.zeros(RECTIFY_RECORD_FLOATS, dtype=np.float64)
    rec[RECTIFY_REC_SRC] = float(src)
    rec[RECTIFY_REC_IR:RECTIFY_REC_IR + 9] = np.linalg.inv(P[:, :3] @ R_rect).reshape(-1)
    rec[RECTIFY_REC_FX:RECTIFY_REC_FX + 4] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    rec[RECTIFY_REC_K1:RECTIFY_REC_K1 + 5] = D[:5]
    return rec


def rectification_records(rectification_data: dict) -> np.ndarray:
    """(2, RECORD_FLOATS) float64: the left camera reading source 0, the right camera reading source 1"""
    r = rectification_data
    return np.stack([camera_record(0, r["K1"], r["D1"], r["R1"], r["P1"]), camera_record(1, r["K2"], r["D2"], r["R2"], r["P2"])])


def population_records(calib_data: dict, image_size: Tuple[int, int], deltas) -> np.ndarray:
    """(2N, RECORD_FLOATS) float64 for the (N,3) roll / pitch / yaw corrections ``deltas``: records 0..N-1 the left camera, N..2N-1 the right"""
    deltas = np.asarray(deltas, dtype=np.float64).reshape(-1, 3)
    recs = [rectification_records(compute_stereo_rectification(calib_data, image_size, create_delta_rotation(*d))) for d in deltas]
    return np.concatenate([np.stack([r[0] for r in recs]), np.stack([r[1] for r in recs])])


def _upload(records: np.ndarray, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(records, dtype=np.float32)).to(device)


def _source(img, device):
    """an (H,W,3) uint8 numpy array is uploaded; a device tensor -- (H,W,3) uint8, (3,H,W) uint8 or fp32 -- is used as it is"""
    import torch
    if isinstance(img, torch.Tensor):
        if not img.is_cuda:
            raise ValueError("s2m2_amd.hip: tensors must be contiguous device tensors")
        return img
    a = np.ascontiguousarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("rectify: a raw image is an (H,W,3) uint8 array")
    return torch.from_numpy(a).to(device)


def _device_of(left, right, device=None):
    import torch
    for t in (left, right):
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise ValueError("s2m2_amd.hip: tensors must be contiguous device tensors")
    for t in (left, right):
        if isinstance(t, torch.Tensor):
            return t.device
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _size(img) -> Tuple[int, int]:
    """(width, height) of an (H,W,3) or (3,H,W) image"""
    s = tuple(img.shape)
    return (s[1], s[0]) if s[2] == 3 else (s[2], s[1])


def rectify_records(left, right, records: np.ndarray, *, out_dtype=None, round: bool = True, device=None):
    """One launch: ``records`` (n, RECORD_FLOATS) over the sources ``left`` (index 0) and ``right`` (index 1) -> (n,3,H,W) device tensor"""
    import torch
    from . import hip
    dev = _device_of(left, right, device)
    srcs = [_source(left, dev), _source(right, dev)]
    w, h = _size(srcs[0])
    out = torch.empty((records.shape[0], 3, h, w), device=dev, dtype=torch.float32 if out_dtype is None else out_dtype)
    hip.rectify(srcs, _upload(records, dev), out, round=round)
    return out


def rectify_images(left_img, right_img, rectification_data: dict):
    """Same arguments as the reference (image_utils.py:108-136): the raw pair -- (H,W,3) uint8 numpy arrays or device tensors -- and the dict of
    ``compute_stereo_rectification`` -> the rectified pair, one launch.  Returned as uint8 device tensors of shape (H,W,3) like the reference's
    arrays; they are views of planar storage, so ``.permute(2, 0, 1)`` is the contiguous (3,H,W) image the model takes."""
    out = rectify_records(left_img, right_img, rectification_records(rectification_data), out_dtype=_torch().uint8)
    return out[0].permute(1, 2, 0), out[1].permute(1, 2, 0)


def _torch():
    import torch
    return torch


def rectify_population(left, right, calib_data: dict, deltas, *, out_dtype=None, round: bool = True, device=None):
    """The raw pair rectified under each of the (N,3) roll / pitch / yaw corrections ``deltas`` -> two (N,3,H,W) device tensors (fp32 by
    default, ``out_dtype=torch.uint8`` for a quarter of the bytes).  The N rectifications are computed on the host in float64, N x 2 records are
    written and ONE launch is issued; the raw images are uploaded at most once (a device tensor passed in is used as it is)."""
    dev = _device_of(left, right, device)
    left, right = _source(left, dev), _source(right, dev)
    records = population_records(calib_data, _size(left), deltas)
    n = records.shape[0] // 2
    out = rectify_records(left, right, records, out_dtype=out_dtype, round=round, device=dev)
    return out[:n], out[n:]


# ------------------------------------------------------------------------------------------------ calibration objective and CEM
def evaluate_sample(model, left, right, calib_data, device, roll_delta, pitch_delta, yaw_delta):
    """Same contract as the reference (calibration/base.py:15-36): the model's mean confidence on the pair rectified under one correction,
    0.0 after printing the error when anything fails."""
    try:
        import torch
        from .utils import compute_confidence_score
        lefts, rights = rectify_population(left, right, calib_data, [[roll_delta, pitch_delta, yaw_delta]], out_dtype=torch.uint8, device=device)
        confidence_score = compute_confidence_score(model, lefts, rights, device)
        return confidence_score if confidence_score is not None else 0.0
    except Exception as e:  # noqa: BLE001  (the reference swallows and reports)
        print(f"Error evaluating sample: {e}")
        return 0.0


def cem_calibration(model, left, right, calib_data, device, **kwargs):
    """Cross-entropy-method search for the roll / pitch / yaw correction of the extrinsic rotation that maximises the model's mean confidence:
    the reference's ``cem_calibration`` (calibration/cem.py) with the same defaults, prints, random draws (the global
    ``np.random.normal(mean, std, (num_samples, 3))`` once per iteration) and result dict.  Each iteration's population is rectified by one
    ``rectify_population`` launch and scored by ``utils.compute_confidence_scores``, to which ``batch=``, ``dist=`` and ``group=`` pass through.
    ``scorer=`` (a callable: (n,3) array of corrections -> n scores) replaces rectification and model.  Beyond the reference's keys the result
    holds ``'iterations'``: per iteration the ``'samples'`` (num_samples+1, 3) and ``'scores'`` it ranked, entry 0 being the current mean."""
    config = {"max_iterations": 5, "num_samples": 20, "num_elite": 3, "initial_std": 0.002, "std_decay": 0.8}
    extra = {k: kwargs.pop(k, None) for k in ("batch", "dist", "group", "scorer")}
    config.update(kwargs)
    print("Starting CEM based online stereo calibration")
    max_iterations, num_samples, num_elite = config["max_iterations"], config["num_samples"], config["num_elite"]
    initial_std, std_decay = config["initial_std"], config["std_decay"]
    if num_elite > num_samples:
        print(f"Warning: num_elite ({num_elite}) cannot be greater than num_samples ({num_samples})")
        print("Setting num_elite to num_samples")
        num_elite = num_samples

    scorer: Optional[Callable] = extra["scorer"]
    if scorer is None:
        import torch
        from .utils import compute_confidence_scores
        dev = _device_of(left, right, device)
        left, right = _source(left, dev), _source(right, dev)                  # the one upload of the calibration

        def scorer(samples: np.ndarray) -> Sequence[float]:
            try:
                lefts, rights = rectify_population(left, right, calib_data, samples, out_dtype=torch.uint8, device=dev)
                return compute_confidence_scores(model, lefts, rights, device, batch=extra["batch"], dist=extra["dist"], group=extra["group"]).tolist()
            except Exception as e:  # noqa: BLE001  (evaluate_sample's contract, for the whole population)
                print(f"Error evaluating sample: {e}")
                return [0.0] * len(samples)

    initial_confidence = float(scorer(np.zeros((1, 3)))[0])
    print(f"Initial confidence: {initial_confidence:.4f}")
    mean_params = np.array([0.0, 0.0, 0.0])
    std_params = np.array([initial_std, initial_std, initial_std])
    current_confidence = initial_confidence
    best_params = mean_params.copy()
    best_confidence = initial_confidence
    history = []
    for iteration in range(max_iterations):
        if best_confidence > 0.98:
            break
        print(f"\nIteration {iteration + 1}/{max_iterations}")
        print(f"Current confidence: {current_confidence:.4f}")
        print(f"Current mean - Roll: {mean_params[0]:.4f}, Pitch: {mean_params[1]:.4f}, Yaw: {mean_params[2]:.4f}")
        print(f"Current std - Roll: {std_params[0]:.4f}, Pitch: {std_params[1]:.4f}, Yaw: {std_params[2]:.4f}")
        samples = np.random.normal(mean_params, std_params, (num_samples, 3))
        scores = [float(s) for s in scorer(samples)]
        sample_scores = [(mean_params, current_confidence)] + [(samples[i], scores[i]) for i in range(num_samples)]
        history.append({"samples": np.stack([s for s, _ in sample_scores]), "scores": np.array([c for _, c in sample_scores])})
        sample_scores.sort(key=lambda x: x[1], reverse=True)
        elite_samples = np.array([sample for sample, _ in sample_scores[:num_elite]])
        elite_scores = [score for _, score in sample_scores[:num_elite]]
        mean_params = np.mean(elite_samples, axis=0)
        std_params = np.maximum(np.std(elite_samples, axis=0) * std_decay, 0.00005)
        if elite_scores[0] > best_confidence:
            best_confidence = elite_scores[0]
            best_params = elite_samples[0].copy()
            current_confidence = elite_scores[0]
        print(f"Best sample confidence: {elite_scores[0]:.4f}")
        print(f"Elite mean - Roll: {mean_params[0]:.4f}, Pitch: {mean_params[1]:.4f}, Yaw: {mean_params[2]:.4f}")

    print("\n" + "=" * 50)
    print("CEM CALIBRATION RESULTS")
    print("=" * 50)
    print(f"Initial confidence: {initial_confidence:.4f}")
    print(f"Final confidence: {best_confidence:.4f}")
    print(f"Confidence improvement: {best_confidence - initial_confidence:+.4f}")
    print(f"Final deltas - Roll: {best_params[0]:.4f}, Pitch: {best_params[1]:.4f}, Yaw: {best_params[2]:.4f}")
    calib_data_new = copy.deepcopy(calib_data)
    calib_data_new["stereo_extrinsic"]["rotation"] = apply_delta_rotation(calib_data["stereo_extrinsic"]["rotation"],
                                                                          euler_to_rotation_matrix(best_params[0], best_params[1], best_params[2]))
    return {"roll_delta": best_params[0], "pitch_delta": best_params[1], "yaw_delta": best_params[2], "initial_confidence": initial_confidence,
            "final_confidence": best_confidence, "calib_data_new": calib_data_new, "iterations": history}
