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
    if disp.dtype != torch.float32 or occ.dtype != torch.float32 or conf.dtype != torch.float32 or disp.dim() != 4 or disp.shape[1] != 1:
        raise ValueError("register: disp / occ / conf must be (B,1,Hp,Wp) fp32 tensors")
    if occ.shape != disp.shape or conf.shape != disp.shape:
        raise ValueError("register: disp, occ and conf must have one shape")
    B, _, Hp, Wp = disp.shape
    d = _h.RegisterDesc()
    c = d.cloud
    if image is not None:
        if image.dtype not in _h._IMG_DT or image.dim() != 4 or image.shape[1] != 3 or image.shape[0] != B:
            raise ValueError("register: image must be a (B,3,H,W) uint8 / fp16 / fp32 tensor")
        if (H is not None and H != image.shape[2]) or (W is not None and W != image.shape[3]):
            raise ValueError("register: H and W differ from the image")
        H, W = image.shape[-2:]
        c.image, c.image_dtype = image.data_ptr(), _h._IMG_DT[image.dtype]
    elif H is None or W is None:
        raise ValueError("register: without an image, H and W are required")
    else:
        c.image_dtype = _h._IMG_DT[torch.uint8]
    R, t = [float(x) for x in R], [float(x) for x in t]
    if len(R) != 9 or len(t) != 3:
        raise ValueError("register: R is nine numbers (row-major), t three")
    c.disp, c.occ, c.conf = disp.data_ptr(), occ.data_ptr(), conf.data_ptr()
    c.B, c.H, c.W, c.Hp, c.Wp, c.unfiltered = B, H, W, Hp, Wp, int(unfiltered)
    c.fx, c.fy, c.cx, c.cy, c.baseline, c.doffs = fx, fy, cx, cy, baseline, doffs
    c.depth_scale, c.depth_trunc, c.conf_min, c.occ_min = depth_scale, depth_trunc, conf_min, occ_min
    d.Ht, d.Wt, d.splat, d.fx_t, d.fy_t, d.cx_t, d.cy_t = Ht, Wt, splat, fx_t, fy_t, cx_t, cy_t
    d.R, d.t = (ctypes.c_double * 9)(*R), (ctypes.c_double * 3)(*t)
    if depth_t is not None:
        _h._mat(depth_t, (B, 1, Ht, Wt), torch.float32, "register: depth_t")
        d.depth_t = depth_t.data_ptr()
    if index_t is not None:
        _h._mat(index_t, (B, 1, Ht, Wt), torch.int32, "register: index_t")
        d.index_t = index_t.data_ptr()
    if image_t is not None:
        if image is None:
            raise ValueError("register: image_t needs the image")
        _h._mat(image_t, (B, 3, Ht, Wt), torch.uint8, "register: image_t")
        d.image_t = image_t.data_ptr()
    if visible is not None:
        _h._mat(visible, (B, 1, H, W), torch.uint8, "register: visible")
        d.visible = visible.data_ptr()
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
    n = int(_h.load().s2m2_register_workspace_bytes(B, Ht, Wt))
    if n == 0:
        raise ValueError(f"register: bad extents B={B} Ht={Ht} Wt={Wt}")
    return n
