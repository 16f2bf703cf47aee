"""3D outputs behind ``S2M2.forward``: validity filter, metric depth and a coloured point cloud, on the device (K15, ``s2m2_cloud``).

The reference's demos do this on the host with numpy and open3d (demo/visualize_3d_middlebury.py:32-52,97-107,
src/s2m2/core/utils/model_utils.py:111-136, the mask of vis_utils.py:62).  Here ``reproject`` takes the padded maps as the forward returns them
and the unpadded left image, and leaves everything on the device: two kernel launches, no synchronisation, capturable in a hipGraph.  Between
its inputs and its outputs this module only allocates; the host reads ``count`` in ``PointCloud.points`` / ``colors`` / ``write_ply`` alone.

A record is 16 bytes -- ``float x, y, z; uint8 r, g, b, a`` (a = 255) -- which is the vertex of a binary little-endian PLY: ``write_ply_records``
writes a record buffer as it is.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import hip

PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n")
RECORD_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])


def write_ply_records(path: str, records) -> int:
    """Host function: ``records`` = n records of 16 bytes (a ``RECORD_DTYPE`` array, an (n,4) int32 array, or bytes) -> binary PLY; returns n."""
    raw = records if isinstance(records, (bytes, bytearray)) else np.ascontiguousarray(records).tobytes()
    if len(raw) % 16:
        raise ValueError("write_ply_records: the buffer is not a whole number of 16-byte records")
    with open(path, "wb") as f:
        f.write((PLY_HEADER % (len(raw) // 16)).encode("ascii"))
        f.write(raw)
    return len(raw) // 16


def read_ply_records(path: str) -> np.ndarray:
    """The inverse of ``write_ply_records`` for files with exactly that vertex layout -> ``RECORD_DTYPE`` array."""
    raw = open(path, "rb").read()
    end = raw.find(b"end_header\n")
    if not raw.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    head = raw[:end].decode("ascii").split("\n")
    n = [int(line.split()[2]) for line in head if line.startswith("element vertex")]
    if "format binary_little_endian 1.0" not in head or len(n) != 1 or [line for line in head if line.startswith("property")] != \
            [line for line in (PLY_HEADER % 0).split("\n") if line.startswith("property")]:
        raise ValueError(f"{path}: not the x y z float / red green blue alpha uchar vertex layout")
    body = raw[end + len(b"end_header\n"):]
    if len(body) != 16 * n[0]:
        raise ValueError(f"{path}: {n[0]} vertices declared, {len(body)} bytes of vertex data")
    return np.frombuffer(body, dtype=RECORD_DTYPE)


def read_calib_file(path: str) -> Dict[str, object]:
    """Middlebury ``calib.txt`` (``key=value`` lines; cam0 / cam1 as ``[a b c; d e f; g h i]``) -> dict with the matrices as (3,3) float64
    arrays and every other value as a float -- the dict the reference demo's function of this name returns."""
    out: Dict[str, object] = {}
    for line in open(path).read().splitlines():
        if "=" not in line:
            continue
        key, val = (s.strip() for s in line.split("=", 1))
        if val.startswith("["):
            out[key] = np.array([float(t) for t in val.strip("[]").replace(";", " ").split()], dtype=np.float64).reshape(3, 3)
        else:
            out[key] = float(val)
    return out


class PointCloud:
    """What ``reproject`` returns: ``records`` (B, capacity, 4) int32 = 16-byte records in raster order, ``count`` (B) int32 on the device (the
    true number of kept pixels, also above capacity), and the optional dense ``depth`` (B,1,H,W) fp32 and ``mask`` (B,1,H,W) uint8."""

    def __init__(self, records: torch.Tensor, count: torch.Tensor, depth: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None):
        self.records, self.count, self.depth, self.mask = records, count, depth, mask

    @property
    def capacity(self) -> int:
        return self.records.shape[1]

    def size(self, b: int = 0) -> int:
        """records stored for pair b: min(count, capacity) -- reads ``count`` on the host (synchronises)"""
        return min(int(self.count[b].item()), self.capacity)

    def points(self, b: int = 0) -> torch.Tensor:
        """(n,3) fp32 strided view of the stored records of pair b"""
        return self.records[b, :self.size(b)].view(torch.float32)[:, :3]

    def colors(self, b: int = 0) -> torch.Tensor:
        """(n,3) uint8 strided view (r, g, b) of the stored records of pair b"""
        return self.records[b, :self.size(b)].view(torch.uint8)[:, 12:15]

    def write_ply(self, path: str, b: int = 0) -> int:
        return write_ply_records(path, self.records[b, :self.size(b)].cpu().numpy())


def reproject(disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, image: torch.Tensor, *, fx: float, cx: float, cy: float,
              baseline: float, doffs: float = 0.0, fy: Optional[float] = None, depth_scale: float = 1000.0,
              depth_trunc: Optional[float] = None, conf_min: float = 0.1, occ_min: float = 0.5, filtered: bool = True,
              capacity: Optional[int] = None, want_depth: bool = False, want_mask: bool = False) -> PointCloud:
    """Padded maps (B,1,Hp,Wp) fp32 + unpadded left image (B,3,H,W) uint8 / fp16 / fp32 in [0,255], contiguous device tensors -> PointCloud.
    The crop of ``image_crop`` is fused (image pixel (v,u) = map pixel (v + (Hp-H)//2, u + (Wp-W)//2)).  fy defaults to fx as in the reference;
    depth_trunc None = 1e9 as in the reference; filtered=False skips the confidence / occlusion test (the reference's first cloud);
    capacity None = H*W records per pair."""
    B = disp.shape[0]
    H, W = image.shape[-2:]
    cap = H * W if capacity is None else int(capacity)
    if cap < 0:
        raise ValueError("reproject: negative capacity")
    dev = disp.device
    records = torch.empty((B, cap, 4), device=dev, dtype=torch.int32)
    count = torch.empty((B,), device=dev, dtype=torch.int32)
    workspace = torch.empty((hip.cloud_workspace_bytes(B, H, W),), device=dev, dtype=torch.uint8)
    depth = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32) if want_depth else None
    mask = torch.empty((B, 1, H, W), device=dev, dtype=torch.uint8) if want_mask else None
    hip.cloud(disp, occ, conf, image, fx=fx, fy=fx if fy is None else fy, cx=cx, cy=cy, baseline=baseline, doffs=doffs,
              depth_scale=depth_scale, depth_trunc=1e9 if depth_trunc is None else depth_trunc, conf_min=conf_min, occ_min=occ_min,
              unfiltered=not filtered, records=records, count=count, workspace=workspace, depth=depth, mask=mask)
    return PointCloud(records, count, depth, mask)
