"""numpy oracle of the 3D output stage (K15, include/s2m2_hip.h: s2m2_cloud), independent of the code under test.

Written from the reference's host code: the validity mask ``(conf > 0.1) * (occ > 0.5)`` (src/s2m2/core/utils/vis_utils.py:62), the filtered
disparity ``disp * valid; [~valid] = -1`` (demo/visualize_3d_middlebury.py:103-104), ``depth = baseline * fx / (disp + doffs); depth[disp <= 0]
= 1e9`` as float32 (src/s2m2/core/utils/model_utils.py:124-126), and open3d's documented conversions behind it:
``RGBDImage.create_from_color_and_depth(depth_scale, depth_trunc)`` divides the depth by depth_scale and sets values at or beyond depth_trunc
to 0; ``PointCloud.create_from_rgbd_image`` walks the image row by row and emits, for every pixel with depth z > 0, the point
``((u - cx) * z / fx, (v - cy) * z / fy, z)`` with the pixel's colour.

The keep / z chain is evaluated in float32 exactly as the header states it (one IEEE rounding per operation: numpy's float32 array arithmetic);
x and y are ALSO given in float64 from the float32 z, the reference point of the error bound of the GPU tests.
"""
import numpy as np

F = np.float32


def crop(m, H, W):
    """image_crop on a (..., Hp, Wp) array: the centred (H, W) window"""
    Hp, Wp = m.shape[-2:]
    oy, ox = (Hp - H) // 2, (Wp - W) // 2
    return m[..., oy:oy + H, ox:ox + W]


def colour_bytes(image):
    """(3,H,W) uint8 / float16 / float32 in [0,255] -> uint8: floats clamped and rounded to nearest even"""
    if image.dtype == np.uint8:
        return image
    return np.rint(np.clip(image.astype(np.float32), 0.0, 255.0)).astype(np.uint8)


def cloud(disp, occ, conf, image, *, fx, fy, cx, cy, baseline, doffs=0.0, depth_scale=1000.0, depth_trunc=None, conf_min=0.1, occ_min=0.5,
          filtered=True):
    """One pair: disp / occ / conf (H,W) float32 ALREADY cropped, image (3,H,W).  Returns a dict:
    keep (H,W) bool; depth (H,W) float32 (z where keep, else 0); index (n) flat pixel indices of the kept pixels in raster order;
    z (n) float32; x32, y32 (n) float32 (the fp32 formula); x64, y64 (n) float64; rgb (n,3) uint8."""
    disp, occ, conf = (np.ascontiguousarray(a, dtype=F) for a in (disp, occ, conf))
    H, W = disp.shape
    if filtered:
        valid = (conf > F(conf_min)) & (occ > F(occ_min))
        d = np.where(valid, disp, F(-1.0))
    else:
        d = disp
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where(d <= 0, F(1e9), F(float(baseline) * float(fx)) / (d + F(doffs))).astype(F)
        z = depth / F(depth_scale)
    keep = (z > 0) & (z < F(1e9 if depth_trunc is None else depth_trunc))
    index = np.flatnonzero(keep.ravel())
    v, u = np.divmod(index, W)
    zk = z.ravel()[index]
    x32 = (u.astype(F) - F(cx)) * zk / F(fx)
    y32 = (v.astype(F) - F(cy)) * zk / F(fy)
    x64 = (u.astype(np.float64) - float(cx)) * zk.astype(np.float64) / float(fx)
    y64 = (v.astype(np.float64) - float(cy)) * zk.astype(np.float64) / float(fy)
    rgb = colour_bytes(image).reshape(3, H * W)[:, index].T
    return dict(keep=keep, depth=np.where(keep, z, F(0)).astype(F), index=index, z=zk, x32=x32, y32=y32, x64=x64, y64=y64,
                rgb=np.ascontiguousarray(rgb))
