"""K22 (``s2m2_segment``, csrc/segment.hip): connected components of the kept pixels and the speckle filter.  The descriptor mirror and the
signatures are in hip.py with all the others (``hip.load()`` binds every symbol there); this module holds the wrappers, which hip.py re-exports
as ``hip.segment``, ``hip.segment_workspace_bytes`` and ``hip.segment_tile``."""
import ctypes
import math
from typing import Optional, Tuple

import torch

from . import hip as _h


def segment(disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, *, H: int, W: int, fx: float, fy: float, cx: float, cy: float,
            baseline: float, doffs: float = 0.0, depth_scale: float = 1000.0, depth_trunc: float = 0.0, conf_min: float = 0.1,
            occ_min: float = 0.5, unfiltered: bool = False, max_jump: float = 1.0, min_size: int = 1, workspace: torch.Tensor,
            label: Optional[torch.Tensor] = None, size: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
            disp_out: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None) -> None:
    """s2m2_segment (K22): the padded maps (B,1,Hp,Wp) fp32 and the image size ``H`` x ``W`` of the fused crop -> the outputs the caller
    allocated: ``label`` (B,1,H,W) int32, ``size`` (B,1,H,W) int32, ``mask`` (B,1,H,W) uint8, ``disp_out`` (B,1,Hp,Wp) fp32 (not ``disp``
    itself), ``stats`` (B,4) int32; ``workspace``: ``segment_workspace_bytes`` bytes.  Thin: no allocation, no synchronisation."""
    if math.isnan(float(max_jump)) or max_jump < 0:
        raise ValueError(f"segment: max_jump must be >= 0 (inf is allowed), got {max_jump}")
    if int(min_size) != min_size or not 1 <= min_size <= 1 << 30:
        raise ValueError(f"segment: min_size must be an integer in 1..2^30, got {min_size}")
    _h._resident("segment", disp, occ, conf, workspace, label, size, mask, disp_out, stats)
    _h._contig("segment", disp, occ, conf, workspace, label, size, mask, disp_out, stats)
    d = _h.SegmentDesc()
    B, H, W = _h._cloud_inputs("segment", d.cloud, disp, occ, conf, None, H, W, fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min,
                               occ_min, unfiltered)
    d.max_jump, d.min_size = float(max_jump), int(min_size)
    d.label = _h._opt(label, (B, 1, H, W), torch.int32, "segment: label")
    d.size = _h._opt(size, (B, 1, H, W), torch.int32, "segment: size")
    d.mask = _h._opt(mask, (B, 1, H, W), torch.uint8, "segment: mask")
    d.disp_out = _h._opt(disp_out, (B, 1, d.cloud.Hp, d.cloud.Wp), torch.float32, "segment: disp_out")
    d.stats = _h._opt(stats, (B, 4), torch.int32, "segment: stats")
    need = segment_workspace_bytes(B, H, W)
    if workspace is None or workspace.nbytes < need:
        raise ValueError(f"segment: a workspace of {need} bytes is required")
    d.workspace = workspace.data_ptr()
    with torch.cuda.device(disp.device):
        _h._check(_h.load().s2m2_segment(ctypes.byref(d), _h._stream()), "s2m2_segment")


def segment_workspace_bytes(B: int, H: int, W: int) -> int:
    return _h._extent_query("s2m2_segment_workspace_bytes", "segment", B=B, H=H, W=W)


def segment_tile(H: int, W: int) -> Tuple[int, int]:
    """(rows, columns) of the tile of K22's local pass at this image size"""
    return _h._extent_query("s2m2_segment_tile_rows", "segment", H=H, W=W), _h._extent_query("s2m2_segment_tile_cols", "segment", H=H, W=W)
