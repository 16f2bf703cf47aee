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
    B, H, W = _h._cloud_inputs("mesh", d.cloud, disp, occ, conf, image, None, None, fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min,
                               occ_min, unfiltered)
    _h._cloud_outputs("mesh", d.cloud, mesh_workspace_bytes, records, count, workspace, depth, mask)
    _h._vec(face_count, B, "mesh: face_count", dtype=torch.int32)
    if faces.dtype != torch.int32 or faces.dim() != 3 or faces.shape[0] != B or faces.shape[2] != 3:
        raise ValueError("mesh: faces must be a (B, face_capacity, 3) int32 tensor")
    d.face_count, d.face_capacity = face_count.data_ptr(), faces.shape[1]
    d.faces = faces.data_ptr() if faces.shape[1] > 0 else None
    d.index = _h._opt(index, (B, 1, H, W), torch.int32, "mesh: index")
    d.max_jump = max_jump
    with torch.cuda.device(disp.device):
        _h._check(_h.load().s2m2_mesh(ctypes.byref(d), _h._stream()), "s2m2_mesh")


def mesh_workspace_bytes(B: int, H: int, W: int) -> int:
    return _h._extent_query("s2m2_mesh_workspace_bytes", "mesh", B=B, H=H, W=W)


def mesh_tile_rows(H: int, W: int) -> int:
    """image rows of one tile of s2m2_mesh's launches (tests sit on the tile boundaries)"""
    return _h._extent_query("s2m2_mesh_tile_rows", "mesh", H=H, W=W)
