"""K29 (``s2m2_smooth``, csrc/smooth.hip): edge-preserving smoothing of the disparity map.  The descriptor mirror and the signatures are in
hip.py with all the others (``hip.load()`` binds every symbol there); this module holds the wrappers, which hip.py re-exports as ``hip.smooth``
and ``hip.smooth_weights``."""
import ctypes
import math
from typing import Optional

import numpy as np
import torch

from . import hip as _h
from .hip_normals import _max_jump, _radius


def _sigma(what: str, name: str, sigma: float) -> float:
    """a width of the filter: finite and > 0"""
    if not (math.isfinite(float(sigma)) and sigma > 0.0):
        raise ValueError(f"{what}: {name} must be finite and > 0, got {sigma}")
    return float(sigma)


def smooth_weights(radius: int, sigma_s: float, sigma_r: float):
    """s2m2_smooth_weights: the tables a call of ``smooth`` with these parameters uses -> (ws (9,) float32 -- entries behind ``radius`` are 0
    --, wr (257,) float32, inv float32).  Host only: no device is touched."""
    what = "smooth_weights"
    ws, wr, inv = np.zeros(9, np.float32), np.zeros(257, np.float32), ctypes.c_float(0.0)
    fp = ctypes.POINTER(ctypes.c_float)
    _h._check(_h.load().s2m2_smooth_weights(_radius(what, radius), _sigma(what, "sigma_s", sigma_s), _sigma(what, "sigma_r", sigma_r),
                                            ws.ctypes.data_as(fp), wr.ctypes.data_as(fp), ctypes.byref(inv)), "s2m2_smooth_weights")
    return ws, wr, np.float32(inv.value)


def smooth(disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, *, H: int, W: int, fx: float, fy: float, cx: float, cy: float,
           baseline: float, doffs: float = 0.0, depth_scale: float = 1000.0, depth_trunc: float = 0.0, conf_min: float = 0.1,
           occ_min: float = 0.5, unfiltered: bool = False, radius: int = 2, sigma_s: float, sigma_r: float, max_jump: float,
           disp_out: Optional[torch.Tensor] = None, taps: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None) -> None:
    """s2m2_smooth (K29): the B padded maps (B,1,Hp,Wp) fp32 with the fused crop H x W and K15's camera and filter numbers -> the outputs the
    caller allocated, each optional, at least one: ``disp_out`` (B,1,Hp,Wp) fp32 (the PADDED map: the smoothed disparity where the pixel is
    kept, -1 elsewhere, the border included; not the input map), ``taps`` (B,1,H,W) int32 neighbours in the pixel's sum, ``count`` (B) int32
    kept pixels.  A bilateral filter over the (2 radius + 1)^2 window with the widths ``sigma_s`` (pixels) and ``sigma_r`` (px of disparity);
    a neighbour enters where its disparity differs from the centre's by at most ``max_jump``.  Thin: no allocation, no synchronisation."""
    what = "smooth"
    _h._resident(what, disp, occ, conf, disp_out, taps, count)
    _h._contig(what, disp, occ, conf, disp_out, taps, count)
    d = _h.SmoothDesc()
    if int(H) != H or int(W) != W:
        raise ValueError(f"{what}: H and W must be integers, got {H} and {W}")
    B, H, W = _h._cloud_inputs(what, d.cloud, disp, occ, conf, None, int(H), int(W), fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc,
                               conf_min, occ_min, unfiltered)
    if not (1 <= H <= disp.shape[2] and 1 <= W <= disp.shape[3]):
        raise ValueError(f"{what}: the crop H={H} W={W} must be positive and no larger than the maps {tuple(disp.shape[2:])}")
    if disp_out is None and taps is None and count is None:
        raise ValueError(f"{what}: no output requested")
    d.disp_out = _h._opt(disp_out, tuple(disp.shape), torch.float32, f"{what}: disp_out")
    d.taps = _h._opt(taps, (B, 1, H, W), torch.int32, f"{what}: taps")
    if count is not None:
        _h._vec(count, B, f"{what}: count", dtype=torch.int32)
        d.count = count.data_ptr()
    d.radius, d.max_jump = _radius(what, radius), _max_jump(what, max_jump)
    d.sigma_s, d.sigma_r = _sigma(what, "sigma_s", sigma_s), _sigma(what, "sigma_r", sigma_r)
    with torch.cuda.device(disp.device):
        _h._check(_h.load().s2m2_smooth(ctypes.byref(d), _h._stream()), "s2m2_smooth")
