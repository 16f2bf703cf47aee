"""K20 (``s2m2_mesh``, csrc/mesh.hip): the surface mesh behind the 3D stage.  The descriptor mirror and the signatures are in hip.py with all the
others (``hip.load()`` binds every symbol there); this module holds the wrappers, which hip.py re-exports as ``hip.mesh``,
``hip.mesh_workspace_bytes`` and ``hip.mesh_tile_rows``."""
import ctypes
from typing import Optional

import torch

from . import hip as _h


def mesh(disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, image: torch.Tensor, *, fx: float, fy: float, cx: float, cy: float,
         baseline: float, doffs: float = 0.0, depth_scale: float = 1000.0, depth_trunc: float = 0.0, conf_min: float = 0.1, occ_min: float = 0.5,
         unfiltered: bool = False, max_jump: float = 1.0, records: torch.Tensor, count: torch.Tensor, faces: torch.Tensor,
         face_count: torch.Tensor, workspace: torch.Tensor, index: Optional[torch.Tensor] = None, depth: Optional[torch.Tensor] = None,
         mask: Optional[torch.Tensor] = None) -> None:
    """s2m2_mesh (K20): the operands of ``cloud`` plus ``faces`` (B, face_capacity, 3) int32 with ``face_count`` (B) int32, a ``workspace`` of
    ``mesh_workspace_bytes`` bytes and the optional dense rank map ``index`` (B,1,H,W) int32.  Thin: no allocation, no synchronisation."""
    _h._resident("mesh", disp, occ, conf, image, records, count, faces, face_count, workspace, index, depth, mask)
    _h._contig("mesh", disp, occ, conf, image, records, count, faces, face_count, workspace, index, depth, mask)
    if records is None or count is None or faces is None or face_count is None:
        raise ValueError("mesh: records, count, faces and face_count are required")
    d = _h.MeshDesc()
    _h._cloud_desc("mesh", d.cloud, mesh_workspace_bytes, disp, occ, conf, image, fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min, occ_min,
                unfiltered, records, count, workspace, depth, mask)
    B, H, W = d.cloud.B, d.cloud.H, d.cloud.W
    _h._vec(face_count, B, "mesh: face_count", dtype=torch.int32)
    if faces.dtype != torch.int32 or faces.dim() != 3 or faces.shape[0] != B or faces.shape[2] != 3:
        raise ValueError("mesh: faces must be a (B, face_capacity, 3) int32 tensor")
    d.face_count, d.face_capacity = face_count.data_ptr(), faces.shape[1]
    d.faces = faces.data_ptr() if faces.shape[1] > 0 else None
    if index is not None:
        _h._mat(index, (B, 1, H, W), torch.int32, "mesh: index")
        d.index = index.data_ptr()
    d.max_jump = max_jump
    with torch.cuda.device(disp.device):
        _h._check(_h.load().s2m2_mesh(ctypes.byref(d), _h._stream()), "s2m2_mesh")


def mesh_workspace_bytes(B: int, H: int, W: int) -> int:
    n = int(_h.load().s2m2_mesh_workspace_bytes(B, H, W))
    if n == 0:
        raise ValueError(f"mesh: bad extents B={B} H={H} W={W}")
    return n


def mesh_tile_rows(H: int, W: int) -> int:
    """image rows of one tile of s2m2_mesh's launches (tests sit on the tile boundaries)"""
    n = int(_h.load().s2m2_mesh_tile_rows(H, W))
    if n == 0:
        raise ValueError(f"mesh: bad extents H={H} W={W}")
    return n
