"""K28 (``s2m2_normals``, csrc/normals.hip): the normal map of the disparity map.  The descriptor mirror and the signature are in hip.py with all
the others (``hip.load()`` binds every symbol there); this module holds the wrapper, which hip.py re-exports as ``hip.normals``."""
import ctypes
import math
from typing import Optional

import torch

from . import hip as _h

NORMALS_MAX_RADIUS = 8


def _radius(what: str, radius: int) -> int:
    """the distance of the neighbours: an integer in 1 .. NORMALS_MAX_RADIUS"""
    if int(radius) != radius or not 1 <= radius <= NORMALS_MAX_RADIUS:
        raise ValueError(f"{what}: radius must be an integer in 1..{NORMALS_MAX_RADIUS}, got {radius}")
    return int(radius)


def _max_jump(what: str, max_jump: float) -> float:
    """the disparity gate: >= 0, +inf allowed, no NaN"""
    if not float(max_jump) >= 0.0:
        raise ValueError(f"{what}: max_jump must be >= 0, got {max_jump}")
    return float(max_jump)


def _min_cos(what: str, min_cos: float) -> float:
    """the view gate: finite and < 1"""
    if not (math.isfinite(float(min_cos)) and min_cos < 1.0):
        raise ValueError(f"{what}: min_cos must be finite and < 1, got {min_cos}")
    return float(min_cos)


def normals(disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, *, H: int, W: int, fx: float, fy: float, cx: float, cy: float,
            baseline: float, doffs: float = 0.0, depth_scale: float = 1000.0, depth_trunc: float = 0.0, conf_min: float = 0.1,
            occ_min: float = 0.5, unfiltered: bool = False, radius: int = 1, max_jump: float = 1.0, min_cos: float = 0.0,
            depth: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None, image: Optional[torch.Tensor] = None,
            count: Optional[torch.Tensor] = None) -> None:
    """s2m2_normals (K28): the B padded maps (B,1,Hp,Wp) fp32 with the fused crop H x W and K15's camera and filter numbers -> the outputs the
    caller allocated, each optional, at least one: ``depth`` (B,1,H,W) fp32 (K15's), ``normals`` (B,3,H,W) fp32 (unit, camera frame, towards the
    camera, 0,0,0 at holes), ``image`` (B,3,H,W) uint8, ``count`` (B) int32 pixels with a normal.  The neighbours lie ``radius`` pixels away and
    are used where the disparity differs by at most ``max_jump * radius``; a normal is kept where its cosine with the direction to the camera
    is at least ``min_cos``.  Thin: no allocation, no synchronisation."""
    what = "normals"
    _h._resident(what, disp, occ, conf, depth, normals, image, count)
    _h._contig(what, disp, occ, conf, depth, normals, image, count)
    d = _h.NormalsDesc()
    if int(H) != H or int(W) != W:
        raise ValueError(f"{what}: H and W must be integers, got {H} and {W}")
    B, H, W = _h._cloud_inputs(what, d.cloud, disp, occ, conf, None, int(H), int(W), fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc,
                               conf_min, occ_min, unfiltered)
    if not (1 <= H <= disp.shape[2] and 1 <= W <= disp.shape[3]):
        raise ValueError(f"{what}: the crop H={H} W={W} must be positive and no larger than the maps {tuple(disp.shape[2:])}")
    if depth is None and normals is None and image is None and count is None:
        raise ValueError(f"{what}: no output requested")
    d.depth = _h._opt(depth, (B, 1, H, W), torch.float32, f"{what}: depth")
    d.normals = _h._opt(normals, (B, 3, H, W), torch.float32, f"{what}: normals")
    d.image = _h._opt(image, (B, 3, H, W), torch.uint8, f"{what}: image")
    if count is not None:
        _h._vec(count, B, f"{what}: count", dtype=torch.int32)
        d.count = count.data_ptr()
    d.radius, d.max_jump, d.min_cos = _radius(what, radius), _max_jump(what, max_jump), _min_cos(what, min_cos)
    with torch.cuda.device(disp.device):
        _h._check(_h.load().s2m2_normals(ctypes.byref(d), _h._stream()), "s2m2_normals")
