"""K23 (``s2m2_voxel``, csrc/voxel.hip): voxel-grid downsampling of K15's point cloud.  The descriptor mirror and the signatures are in hip.py
with all the others (``hip.load()`` binds every symbol there); this module holds the wrappers, which hip.py re-exports as ``hip.voxel``,
``hip.voxel_workspace_bytes``, ``hip.voxel_tile_rows``, ``hip.voxel_slots`` and ``hip.voxel_home_slot``."""
import ctypes
import math
from typing import Optional

import torch

from . import hip as _h


def voxel(disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, image: torch.Tensor, *, fx: float, fy: float, cx: float, cy: float,
          baseline: float, doffs: float = 0.0, depth_scale: float = 1000.0, depth_trunc: float = 0.0, conf_min: float = 0.1,
          occ_min: float = 0.5, unfiltered: bool = False, voxel_size: float, max_voxels: int, workspace: torch.Tensor,
          records: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
          index: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None) -> None:
    """s2m2_voxel (K23): the padded maps (B,1,Hp,Wp) fp32 and the UNPADDED left image (B,3,H,W) uint8 / fp16 / fp32 -> the outputs the caller
    allocated: ``records`` (B, capacity, 4) int32 = 16-byte voxel records in the raster order of their first points, ``weights``
    (B, capacity) int32, ``count`` (B) int32, ``index`` (B,1,H,W) int32, ``stats`` (B,4) int32; ``workspace``: ``voxel_workspace_bytes``
    bytes.  ``records`` and ``weights`` share one capacity.  Thin: no allocation, no synchronisation."""
    if not (math.isfinite(float(voxel_size)) and voxel_size > 0):
        raise ValueError(f"voxel: voxel_size must be finite and > 0, got {voxel_size}")
    if int(max_voxels) != max_voxels or not 1 <= max_voxels <= 1 << 29:
        raise ValueError(f"voxel: max_voxels must be an integer in 1..2^29, got {max_voxels}")
    _h._resident("voxel", disp, occ, conf, image, workspace, records, weights, count, index, stats)
    _h._contig("voxel", disp, occ, conf, image, workspace, records, weights, count, index, stats)
    d = _h.VoxelDesc()
    B, H, W = _h._cloud_inputs("voxel", d.cloud, disp, occ, conf, image, None, None, fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc,
                               conf_min, occ_min, unfiltered)
    d.voxel_size, d.max_voxels = float(voxel_size), int(max_voxels)
    capacity = None
    if records is not None:
        if records.dtype != torch.int32 or records.dim() != 3 or records.shape[0] != B or records.shape[2] != 4:
            raise ValueError("voxel: records must be a (B, capacity, 4) int32 tensor")
        capacity = records.shape[1]
    if weights is not None:
        if weights.dtype != torch.int32 or weights.dim() != 2 or weights.shape[0] != B or capacity not in (None, weights.shape[1]):
            raise ValueError("voxel: weights must be a (B, capacity) int32 tensor, with the capacity of records")
        capacity = weights.shape[1]
    d.capacity = capacity or 0
    if capacity:
        d.records, d.weights = _h._ptr(records), _h._ptr(weights)
    d.count = _h._opt(count, (B,), torch.int32, "voxel: count")
    d.index = _h._opt(index, (B, 1, H, W), torch.int32, "voxel: index")
    d.stats = _h._opt(stats, (B, 4), torch.int32, "voxel: stats")
    need = voxel_workspace_bytes(B, H, W, max_voxels)
    if workspace is None or workspace.nbytes < need:
        raise ValueError(f"voxel: a workspace of {need} bytes is required")
    d.workspace = workspace.data_ptr()
    with torch.cuda.device(disp.device):
        _h._check(_h.load().s2m2_voxel(ctypes.byref(d), _h._stream()), "s2m2_voxel")


def voxel_workspace_bytes(B: int, H: int, W: int, max_voxels: int) -> int:
    return _h._extent_query("s2m2_voxel_workspace_bytes", "voxel", B=B, H=H, W=W, max_voxels=max_voxels)


def voxel_tile_rows(H: int, W: int) -> int:
    """rows of a raster tile of K23's walk (K15's tile) at this image size"""
    return _h._extent_query("s2m2_voxel_tile_rows", "voxel", H=H, W=W)


def voxel_slots(max_voxels: int) -> int:
    """slots of a pair's hash table: the smallest power of two >= 2 * max_voxels (include/s2m2_hip.h, K23)"""
    if int(max_voxels) != max_voxels or not 1 <= max_voxels <= 1 << 29:
        raise ValueError(f"voxel: max_voxels must be an integer in 1..2^29, got {max_voxels}")
    return max(2, 1 << (2 * int(max_voxels) - 1).bit_length())


def voxel_home_slot(ix: int, iy: int, iz: int, slots: int) -> int:
    """where the probe chain of voxel (ix, iy, iz) starts in a table of ``slots`` slots (host code of the library)"""
    s = int(_h.load().s2m2_voxel_home_slot(ix, iy, iz, slots))
    if s < 0:
        raise ValueError(f"voxel: bad arguments ix={ix} iy={iy} iz={iz} slots={slots}")
    return s
