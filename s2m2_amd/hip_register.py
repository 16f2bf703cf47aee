"""K21 (``s2m2_register``, csrc/register.hip): the depth map registered to a second camera.  The descriptor mirror and the signatures are in hip.py
with all the others (``hip.load()`` binds every symbol there); this module holds the wrappers, which hip.py re-exports as ``hip.register`` and
``hip.register_workspace_bytes``."""
import ctypes
from typing import Optional, Sequence

import torch

from . import hip as _h


def register(disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, image: Optional[torch.Tensor], *, H: Optional[int] = None,
             W: Optional[int] = None, fx: float, fy: float, cx: float, cy: float, baseline: float, doffs: float = 0.0, depth_scale: float = 1000.0,
             depth_trunc: float = 0.0, conf_min: float = 0.1, occ_min: float = 0.5, unfiltered: bool = False, Ht: int, Wt: int, splat: int = 2,
             fx_t: float, fy_t: float, cx_t: float, cy_t: float, R: Sequence[float], t: Sequence[float], workspace: torch.Tensor,
             depth_t: Optional[torch.Tensor] = None, index_t: Optional[torch.Tensor] = None, image_t: Optional[torch.Tensor] = None,
             visible: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None) -> None:
    """s2m2_register (K21): the padded maps (B,1,Hp,Wp) fp32 and the UNPADDED left image (B,3,H,W) uint8 / fp16 / fp32 (None: pass ``H`` and
    ``W``; no ``image_t`` then) -> the outputs the caller allocated, in the target camera ``Ht`` x ``Wt`` with intrinsics ``fx_t, fy_t, cx_t,
    cy_t`` and the pose ``R`` (nine numbers, row-major, source -> target) and ``t`` (three, in the unit of z): ``depth_t`` (B,1,Ht,Wt) fp32,
    ``index_t`` (B,1,Ht,Wt) int32, ``image_t`` (B,3,Ht,Wt) uint8, ``visible`` (B,1,H,W) uint8, ``count`` (B) int32; ``workspace``:
    ``register_workspace_bytes`` bytes.  Thin: no allocation, no synchronisation."""
    _h._resident("register", disp, occ, conf, image, workspace, depth_t, index_t, image_t, visible, count)
    _h._contig("register", disp, occ, conf, image, workspace, depth_t, index_t, image_t, visible, count)
    d = _h.RegisterDesc()
    B, H, W = _h._cloud_inputs("register", d.cloud, disp, occ, conf, image, H, W, fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min,
                               occ_min, unfiltered)
    R, t = [float(x) for x in R], [float(x) for x in t]
    if len(R) != 9 or len(t) != 3:
        raise ValueError("register: R is nine numbers (row-major), t three")
    d.Ht, d.Wt, d.splat, d.fx_t, d.fy_t, d.cx_t, d.cy_t = Ht, Wt, splat, fx_t, fy_t, cx_t, cy_t
    d.R, d.t = (ctypes.c_double * 9)(*R), (ctypes.c_double * 3)(*t)
    d.depth_t = _h._opt(depth_t, (B, 1, Ht, Wt), torch.float32, "register: depth_t")
    d.index_t = _h._opt(index_t, (B, 1, Ht, Wt), torch.int32, "register: index_t")
    if image_t is not None and image is None:
        raise ValueError("register: image_t needs the image")
    d.image_t = _h._opt(image_t, (B, 3, Ht, Wt), torch.uint8, "register: image_t")
    d.visible = _h._opt(visible, (B, 1, H, W), torch.uint8, "register: visible")
    if count is not None:
        _h._vec(count, B, "register: count", dtype=torch.int32)
        d.count = count.data_ptr()
    need = register_workspace_bytes(B, Ht, Wt)
    if workspace is None or workspace.nbytes < need:
        raise ValueError(f"register: a workspace of {need} bytes is required")
    d.workspace = workspace.data_ptr()
    with torch.cuda.device(disp.device):
        _h._check(_h.load().s2m2_register(ctypes.byref(d), _h._stream()), "s2m2_register")


def register_workspace_bytes(B: int, Ht: int, Wt: int) -> int:
    return _h._extent_query("s2m2_register_workspace_bytes", "register", B=B, Ht=Ht, Wt=Wt)
