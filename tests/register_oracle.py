"""numpy oracle of K21 (include/s2m2_hip.h: s2m2_register), written from the header's comment block and independent of the code under test.

keep, z, x and y are those of tests/cloud_oracle.py (K15's chain).  Everything behind them -- transform, projection, footprint origin -- is
float32 array arithmetic, one IEEE rounding per operation exactly as the header lists them, so the GPU tests compare bit for bit: there is no
threshold for a value to sit near.  The z-buffer is ``np.minimum.at`` over the 64-bit keys, once per footprint offset.
"""
import numpy as np

import cloud_oracle

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def register(disp, occ, conf, image, *, Ht, Wt, fx_t, fy_t, cx_t, cy_t, R=None, t=None, splat=2, **cloud_kw):
    """One pair: disp / occ / conf (H,W) float32 ALREADY cropped, image (3,H,W) or None; ``cloud_kw``: the keywords of ``cloud_oracle.cloud``.
    Returns a dict: depth_t (Ht,Wt) float32, index_t (Ht,Wt) int32, image_t (3,Ht,Wt) uint8 (None without image), visible (H,W) uint8,
    count int, keep (H,W) bool and depth (H,W) float32 (K15's, in the source camera)."""
    H, W = disp.shape
    o = cloud_oracle.cloud(disp, occ, conf, np.zeros((3, H, W), np.uint8) if image is None else image, **cloud_kw)
    index, z, x, y = o["index"], o["z"], o["x32"], o["y32"]
    r = (np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3)).astype(F)
    tt = (np.zeros(3) if t is None else np.asarray(t, dtype=np.float64).reshape(3)).astype(F)
    with np.errstate(all="ignore"):
        X = ((r[0, 0] * x + r[0, 1] * y) + r[0, 2] * z) + tt[0]
        Y = ((r[1, 0] * x + r[1, 1] * y) + r[1, 2] * z) + tt[1]
        Z = ((r[2, 0] * x + r[2, 1] * y) + r[2, 2] * z) + tt[2]
        assert X.dtype == F and Z.dtype == F
        ok = (Z > 0) & np.isfinite(Z)
        up = (F(fx_t) * X) / Z + F(cx_t)
        vp = (F(fy_t) * Y) / Z + F(cy_t)
        c = F((splat - 2) / 2)
        fu, fv = np.floor(up - c), np.floor(vp - c)
        assert fu.dtype == F
        ok &= (fu >= F(-splat)) & (fu < F(Wt)) & (fv >= F(-splat)) & (fv < F(Ht))
    index, Z = index[ok], np.ascontiguousarray(Z[ok])
    fu, fv = fu[ok].astype(np.int64), fv[ok].astype(np.int64)
    keys = (Z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index.astype(np.uint64)
    zbuf = np.full(Ht * Wt, EMPTY, dtype=np.uint64)
    for dy in range(splat):
        for dx in range(splat):
            tv, tu = fv + dy, fu + dx
            m = (tv >= 0) & (tv < Ht) & (tu >= 0) & (tu < Wt)
            np.minimum.at(zbuf, tv[m] * Wt + tu[m], keys[m])
    hit = zbuf != EMPTY
    depth_t = np.where(hit, (zbuf >> np.uint64(32)).astype(np.uint32).view(F), F(0)).astype(F).reshape(Ht, Wt)
    index_t = np.where(hit, (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32).reshape(Ht, Wt)
    visible = np.zeros(H * W, dtype=np.uint8)
    visible[index_t[index_t >= 0]] = 1
    image_t = None
    if image is not None:
        rgb = cloud_oracle.colour_bytes(image).reshape(3, H * W)
        image_t = np.where(hit, rgb[:, np.maximum(index_t.ravel(), 0)], 0).astype(np.uint8).reshape(3, Ht, Wt)
    return dict(depth_t=depth_t, index_t=index_t, image_t=image_t, visible=visible.reshape(H, W), count=int(hit.sum()), keep=o["keep"],
                depth=o["depth"])


def right_view_scene(H, W):
    """NOT part of the oracle: the analytic expectation of the right-view tests, built without any projection arithmetic.
    An integer-disparity scene and what the rectified right camera sees of it, painted far to near: a background at 8 px and a rectangle
    at 40 px (rows H/4 .. 3H/4, columns W/2 .. 3W/4).  doffs = 0 and cx1 = cx0, so a pixel of disparity d lands exactly d columns to the left.
    Returns disp (H,W) float32, the expected index_t (H,W) int32 and the expected visible (H,W) uint8."""
    disp = np.full((H, W), 8.0, dtype=F)
    r0, r1, c0, c1 = H // 4, 3 * H // 4, W // 2, 3 * W // 4
    disp[r0:r1, c0:c1] = 40.0
    own = np.arange(H * W, dtype=np.int32).reshape(H, W)
    index = np.full((H, W), -1, dtype=np.int32)
    index[:, :W - 8] = own[:, 8:]                                    # far first: the background, every pixel shifted by 8 ...
    index[r0:r1, c0 - 8:c1 - 8] = -1                                 # ... except where the rectangle stood in the left view: nothing behind it was seen
    index[r0:r1, c0 - 40:c1 - 40] = own[r0:r1, c0:c1]                # near last: the rectangle, shifted by 40, over whatever is there
    visible = np.zeros(H * W, dtype=np.uint8)
    visible[index[index >= 0]] = 1
    return disp, index, visible.reshape(H, W)
