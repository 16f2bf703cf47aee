"""float64 numpy oracle of the rectifier (K16) and of the host algorithm in front of it, written from the OpenCV documentation
(stereoRectify with CALIB_ZERO_DISPARITY and alpha = 0, initUndistortRectifyMap, undistortPoints, remap with INTER_LINEAR / BORDER_CONSTANT 0)
and the steps of Bouguet's algorithm.  It imports nothing from the package under test.

Conventions where OpenCV versions differ: the four corners and the 9 x 9 grid span 0 .. nx-1, 0 .. ny-1; the border distances of the
alpha = 0 scaling are measured to nx, ny; the point undistortion inside stereo_rectify is the fixed-point iteration stopped at a largest step
below 1e-5 (undistort_fixed_point), the rule of the prototype whose figures the CPU test records."""
import xml.etree.ElementTree as ET

import numpy as np


def parse_xml(path):
    root = ET.parse(path).getroot()
    nums = lambda e: np.array([float(t) for t in e.text.split(",")], dtype=np.float64)
    out = {}
    for key, tag in (("left", "distorted_left_intrinsic"), ("right", "distorted_right_intrinsic"), ("rgb", "distorted_rgb_intrinsic")):
        e = root.find(tag)
        out[key] = {k: float(e.find(k).text) for k in ("fx", "fy", "cx", "cy")}
        out[key]["distortion"] = nums(e.find("dist"))
    for key in ("stereo_extrinsic", "left2rgb"):
        e = root.find(key)
        out[key] = {"rotation": nums(e.find("rotation")).reshape(3, 3), "translation": nums(e.find("translation"))}
    return out


def window_calib(calib, x0, y0):
    """the camera of an image window at offset (x0, y0): cx -= x0, cy -= y0, everything else unchanged"""
    import copy
    c = copy.deepcopy(calib)
    for side in ("left", "right"):
        c[side]["cx"] -= x0
        c[side]["cy"] -= y0
    return c


def euler_xyz(roll, pitch, yaw):
    """extrinsic x-y-z: rotate about the fixed x axis, then y, then z -> Rz @ Ry @ Rx"""
    cr, sr, cp, sp, cw, sw = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]], dtype=np.float64)
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]], dtype=np.float64)
    Rz = np.array([[cw, -sw, 0], [sw, cw, 0], [0, 0, 1]], dtype=np.float64)
    return Rz @ Ry @ Rx


def rot(v):
    """rotation vector -> matrix (Rodrigues)"""
    v = np.asarray(v, dtype=np.float64)
    th = np.linalg.norm(v)
    if th < 1e-300:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def rotvec(R):
    """matrix -> rotation vector (angles below pi)"""
    a = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = np.linalg.norm(a), 0.5 * (np.trace(R) - 1.0)
    if s < 1e-300:
        return a
    return a / s * np.arctan2(s, c)


def distort(x, y, D):
    """normalised undistorted -> normalised distorted coordinates (k1 k2 p1 p2 k3)"""
    k1, k2, p1, p2, k3 = D
    r2 = x * x + y * y
    kr = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    return x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y


def undistort_normalised(xd, yd, D):
    """the exact inverse of ``distort`` (residual at rounding level): OpenCV's fixed-point iteration as the start, Newton steps to finish"""
    k1, k2, p1, p2, k3 = D
    xd, yd = np.asarray(xd, dtype=np.float64), np.asarray(yd, dtype=np.float64)
    x, y = xd.copy(), yd.copy()
    for _ in range(10):
        r2 = x * x + y * y
        ic = 1.0 / (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3)
        x, y = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) * ic, (yd - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) * ic
    h = 1e-7
    for _ in range(50):
        fx, fy = distort(x, y, D)
        ex, ey = fx - xd, fy - yd
        if max(np.abs(ex).max(), np.abs(ey).max()) < 4e-16:
            break
        ax, ay = distort(x + h, y, D)
        bx, by = distort(x, y + h, D)
        j00, j10, j01, j11 = (ax - fx) / h, (ay - fy) / h, (bx - fx) / h, (by - fy) / h
        det = j00 * j11 - j01 * j10
        x, y = x - (j11 * ex - j01 * ey) / det, y - (j00 * ey - j10 * ex) / det
    return x, y


def undistort_fixed_point(xd, yd, D, tol=1e-5, max_iter=1000):
    """the inverse of ``distort`` as the host algorithm of the rectification iterates it: OpenCV's fixed-point step, repeated until the largest
    step over the point set is below ``tol`` (normalised coordinates).  The points it is used for only choose f and c"""
    k1, k2, p1, p2, k3 = D
    xd, yd = np.asarray(xd, dtype=np.float64), np.asarray(yd, dtype=np.float64)
    x, y = xd.copy(), yd.copy()
    for _ in range(max_iter):
        r2 = x * x + y * y
        ic = 1.0 / (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3)
        xn, yn = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) * ic, (yd - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) * ic
        step = max(np.abs(xn - x).max(), np.abs(yn - y).max())
        x, y = xn, yn
        if step < tol:
            break
    return x, y


def undistort_points(pts, K, D, R=None, P=None, exact=True):
    """pixel coordinates (n,2) of the raw camera -> undistorted, optionally rotated by R and projected by P[:, :3] (cv2.undistortPoints);
    ``exact``: the inverse at rounding level (property tests), otherwise the fixed-point iteration of the host algorithm"""
    inverse = undistort_normalised if exact else undistort_fixed_point
    x, y = inverse((pts[:, 0] - K[0, 2]) / K[0, 0], (pts[:, 1] - K[1, 2]) / K[1, 1], D)
    if R is not None:
        q = R @ np.stack([x, y, np.ones_like(x)])
        x, y = q[0] / q[2], q[1] / q[2]
    if P is not None:
        x, y = P[0, 0] * x + P[0, 2], P[1, 1] * y + P[1, 2]
    return np.stack([x, y], axis=1)


def camera_matrix(c):
    return np.array([[c["fx"], 0, c["cx"]], [0, c["fy"], c["cy"]], [0, 0, 1]], dtype=np.float64)


def stereo_rectify(calib, image_size, delta_R=None):
    nx, ny = image_size
    K = [camera_matrix(calib["left"]), camera_matrix(calib["right"])]
    D = [np.asarray(calib["left"]["distortion"], dtype=np.float64), np.asarray(calib["right"]["distortion"], dtype=np.float64)]
    R = np.asarray(calib["stereo_extrinsic"]["rotation"], dtype=np.float64)
    T = np.asarray(calib["stereo_extrinsic"]["translation"], dtype=np.float64)
    if delta_R is not None:
        R = R @ delta_R
    # 1-4: split the rotation between the cameras, then turn the baseline onto the dominant axis
    r_r = rot(-0.5 * rotvec(R))
    t = r_r @ T
    idx = 0 if abs(t[0]) > abs(t[1]) else 1
    uu = np.zeros(3)
    uu[idx] = 1.0 if t[idx] > 0 else -1.0
    ww = np.cross(t, uu)
    nw = np.linalg.norm(ww)
    if nw > 0:
        ww = ww * (np.arccos(abs(t[idx]) / np.linalg.norm(t)) / nw)
    wR = rot(ww)
    Rk = [wR @ r_r.T, wR @ r_r]
    t = Rk[1] @ T
    # 5: new focal length
    f = np.inf
    for k in range(2):
        fc = K[k][idx ^ 1, idx ^ 1]
        if D[k][0] < 0:
            fc *= 1 + D[k][0] * (nx * nx + ny * ny) / (4 * fc * fc)
        f = min(f, fc)
    # 6: principal points
    corners = np.array([[0, 0], [nx - 1, 0], [0, ny - 1], [nx - 1, ny - 1]], dtype=np.float64)
    cc = []
    for k in range(2):
        q = undistort_points(corners, K[k], D[k], R=Rk[k], exact=False) * f
        cc.append(np.array([(nx - 1) / 2, (ny - 1) / 2]) - q.mean(axis=0))
    c = 0.5 * (cc[0] + cc[1])
    # 8: alpha = 0
    g = np.linspace(0, 1, 9)
    gx, gy = np.meshgrid(g * (nx - 1), g * (ny - 1))
    grid = np.stack([gx.ravel(), gy.ravel()], axis=1)
    newA = np.array([[f, 0, c[0]], [0, f, c[1]], [0, 0, 1]])
    s = 0.0
    for k in range(2):
        q = undistort_points(grid, K[k], D[k], R=Rk[k], P=newA, exact=False).reshape(9, 9, 2)
        x0, x1, y0, y1 = q[:, 0, 0].max(), q[:, -1, 0].min(), q[0, :, 1].max(), q[-1, :, 1].min()
        s = max(s, c[0] / (c[0] - x0), c[1] / (c[1] - y0), (nx - c[0]) / (x1 - c[0]), (ny - c[1]) / (y1 - c[1]))
    f = f * s
    P1 = np.array([[f, 0, c[0], 0], [0, f, c[1], 0], [0, 0, 1, 0]], dtype=np.float64)
    P2 = P1.copy()
    P2[idx, 3] = t[idx] * f
    Q = np.array([[1, 0, 0, -c[0]], [0, 1, 0, -c[1]], [0, 0, 0, f], [0, 0, -1.0 / t[idx], 0.0]], dtype=np.float64)
    return dict(K1=K[0], D1=D[0], K2=K[1], D2=D[1], R=R, T=T, R1=Rk[0], R2=Rk[1], P1=P1, P2=P2, Q=Q)


def make_record(src, K, D, Rk, P):
    """the 19 values of a K16 record (float64; the caller rounds to fp32): source index, iR row-major, fx fy cx cy, k1 k2 p1 p2 k3"""
    iR = np.linalg.inv(P[:, :3] @ Rk)
    return np.concatenate([[float(src)], iR.ravel(), [K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.asarray(D, dtype=np.float64)[:5]])


def maps(rec, Hd, Wd, dtype=np.float64):
    """mapx, mapy of every output pixel as initUndistortRectifyMap documents them, evaluated in ``dtype`` from the record rounded to ``dtype``"""
    r = np.asarray(rec).astype(dtype)
    iR, (fx, fy, cx, cy), (k1, k2, p1, p2, k3) = r[1:10].reshape(3, 3), r[10:14], r[14:19]
    u = np.arange(Wd, dtype=dtype)[None, :]
    v = np.arange(Hd, dtype=dtype)[:, None]
    X = iR[0, 0] * u + iR[0, 1] * v + iR[0, 2]
    Y = iR[1, 0] * u + iR[1, 1] * v + iR[1, 2]
    W = iR[2, 0] * u + iR[2, 1] * v + iR[2, 2]
    x, y = X / W, Y / W
    r2 = x * x + y * y
    kr = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    two = dtype(2)
    xd = x * kr + two * p1 * x * y + p2 * (r2 + two * x * x)
    yd = y * kr + p1 * (r2 + two * y * y) + two * p2 * x * y
    mx, my = fx * xd + cx, fy * yd + cy
    assert mx.dtype == dtype and my.dtype == dtype
    return mx, my


def remap(img, mx, my, dtype=np.float64):
    """exact bilinear sampling of the planar image (3,H,W) at (mx, my), taps outside the image contribute 0; unrounded, in ``dtype``"""
    _, H, W = img.shape
    img = img.astype(dtype)
    ok = np.isfinite(mx) & np.isfinite(my) & (mx > -1) & (mx < W) & (my > -1) & (my < H)
    mxs, mys = np.where(ok, mx, 0).astype(dtype), np.where(ok, my, 0).astype(dtype)
    x0f, y0f = np.floor(mxs), np.floor(mys)
    wx, wy = (mxs - x0f)[None], (mys - y0f)[None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)

    def tap(yy, xx):
        inside = ok & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return np.where(inside[None], img[:, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], dtype(0))

    one = dtype(1)
    return ((one - wy) * ((one - wx) * tap(y0, x0) + wx * tap(y0, x0 + 1)) + wy * ((one - wx) * tap(y0 + 1, x0) + wx * tap(y0 + 1, x0 + 1)))


def levels(x):
    """rounded to the nearest integer level, ties to even"""
    return np.rint(x)


def rectify(img, rec, Hd, Wd, dtype=np.float64):
    mx, my = maps(rec, Hd, Wd, dtype)
    return remap(img, mx, my, dtype)
