"""K24 (``s2m2_tsdf_integrate`` / ``s2m2_tsdf_extract``, csrc/tsdf.hip): depth maps fused into a TSDF volume, and the volume's surface points;
K25 (``s2m2_tsdf_mesh``, csrc/tsdf_mesh.hip): that surface as a triangle mesh; K26 (``s2m2_tsdf_raycast``, csrc/tsdf_raycast.hip): the volume
ray-cast into the depth, gradient and colour maps of a camera; K27 (``s2m2_tsdf_track``, csrc/tsdf_track.hip): the camera tracked against those
maps.
The descriptor mirrors and the signatures are in hip.py with all the others (``hip.load()`` binds every symbol there); this module holds the
wrappers, which hip.py re-exports as ``hip.tsdf_integrate``, ``hip.tsdf_extract``, ``hip.tsdf_mesh``, ``hip.tsdf_raycast``,
``hip.tsdf_raycast_steps``, ``hip.tsdf_track``, ``hip.tsdf_track_workspace_bytes``, ``hip.tsdf_workspace_bytes``,
``hip.tsdf_mesh_workspace_bytes`` and ``hip.tsdf_tile_voxels``."""
import ctypes
import math
from typing import Optional, Sequence, Tuple

import torch

from . import hip as _h


def _volume(what: str, volume: torch.Tensor) -> Tuple[int, int, int]:
    """the volume operand: a contiguous (Nz, Ny, Nx, 4) int32 tensor = 16 bytes per voxel, voxel (i, j, k) at [k, j, i] -> (Nx, Ny, Nz)"""
    if volume is None or volume.dtype != torch.int32 or volume.dim() != 4 or volume.shape[3] != 4 or not volume.is_contiguous():
        raise ValueError(f"{what}: the volume must be a contiguous (Nz, Ny, Nx, 4) int32 tensor")
    Nz, Ny, Nx = volume.shape[:3]
    if min(Nx, Ny, Nz) < 1 or Nx * Ny * Nz >= 1 << 29:
        raise ValueError(f"{what}: bad dims Nx={Nx} Ny={Ny} Nz={Nz} (positive, Nx*Ny*Nz < 2^29)")
    return Nx, Ny, Nz


def _placement(what: str, origin: Sequence[float], voxel_size: float):
    """the grid's placement: three finite numbers and a finite size > 0 -> (ctypes origin, voxel_size)"""
    origin = [float(x) for x in origin]
    if len(origin) != 3 or not all(math.isfinite(x) for x in origin):
        raise ValueError(f"{what}: origin is three finite numbers")
    if not (math.isfinite(float(voxel_size)) and voxel_size > 0):
        raise ValueError(f"{what}: voxel_size must be finite and > 0, got {voxel_size}")
    return (ctypes.c_double * 3)(*origin), float(voxel_size)


def tsdf_integrate(volume: torch.Tensor, disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, image: torch.Tensor, poses: torch.Tensor, *,
                   fx: float, fy: float, cx: float, cy: float, baseline: float, doffs: float = 0.0, depth_scale: float = 1000.0,
                   depth_trunc: float = 0.0, conf_min: float = 0.1, occ_min: float = 0.5, unfiltered: bool = False, origin: Sequence[float],
                   voxel_size: float, trunc: float, max_weight: int = 64, carve: bool = False) -> None:
    """s2m2_tsdf_integrate (K24): the B padded maps (B,1,Hp,Wp) fp32, the UNPADDED left images (B,3,H,W) uint8 / fp16 / fp32 and the DEVICE
    pose buffer ``poses`` (B,12) fp32 ([R | t] row-major, world -> camera) are fused into ``volume`` (Nz,Ny,Nx,4) int32 in place, pair by
    pair in the order of the batch.  Thin: no allocation, no synchronisation."""
    _h._resident("tsdf_integrate", volume, disp, occ, conf, image, poses)
    _h._contig("tsdf_integrate", volume, disp, occ, conf, image, poses)
    d = _h.TsdfDesc()
    d.Nx, d.Ny, d.Nz = _volume("tsdf_integrate", volume)
    if image is None:
        raise ValueError("tsdf_integrate: the image is required")
    B, _, _ = _h._cloud_inputs("tsdf_integrate", d.cloud, disp, occ, conf, image, None, None, fx, fy, cx, cy, baseline, doffs, depth_scale,
                               depth_trunc, conf_min, occ_min, unfiltered)
    _h._mat(poses, (B, 12), torch.float32, "tsdf_integrate: poses")
    d.origin, d.voxel_size = _placement("tsdf_integrate", origin, voxel_size)
    if not (math.isfinite(float(trunc)) and trunc > 0):
        raise ValueError(f"tsdf_integrate: trunc must be finite and > 0, got {trunc}")
    if int(max_weight) != max_weight or not 1 <= max_weight <= 32767:
        raise ValueError(f"tsdf_integrate: max_weight must be an integer in 1..32767, got {max_weight}")
    d.trunc, d.max_weight, d.carve = float(trunc), int(max_weight), int(bool(carve))
    d.volume, d.poses = volume.data_ptr(), poses.data_ptr()
    with torch.cuda.device(disp.device):
        _h._check(_h.load().s2m2_tsdf_integrate(ctypes.byref(d), _h._stream()), "s2m2_tsdf_integrate")


def _extract_operands(what: str, d, volume: torch.Tensor, origin, voxel_size, min_weight, records, gradients, count) -> Optional[int]:
    """the extraction descriptor ``d`` (a TsdfExtractDesc) but for its workspace, from the operands that tsdf_extract and tsdf_mesh share
    -> the capacity of records / gradients (None: neither was passed)"""
    d.Nx, d.Ny, d.Nz = _volume(what, volume)
    d.origin, d.voxel_size = _placement(what, origin, voxel_size)
    if int(min_weight) != min_weight or min_weight < 1:
        raise ValueError(f"{what}: min_weight must be an integer >= 1, got {min_weight}")
    d.min_weight = int(min_weight)
    capacity = None
    if records is not None:
        if records.dtype != torch.int32 or records.dim() != 2 or records.shape[1] != 4:
            raise ValueError(f"{what}: records must be a (capacity, 4) int32 tensor")
        capacity = records.shape[0]
    if gradients is not None:
        if gradients.dtype != torch.float32 or gradients.dim() != 2 or gradients.shape[1] != 3 or capacity not in (None, gradients.shape[0]):
            raise ValueError(f"{what}: gradients must be a (capacity, 3) fp32 tensor, with the capacity of records")
        capacity = gradients.shape[0]
    d.capacity = capacity or 0
    if capacity:
        d.records, d.gradients = _h._ptr(records), _h._ptr(gradients)
    if count is not None:
        _h._vec(count, 1, f"{what}: count", dtype=torch.int32)
        d.count = count.data_ptr()
    d.volume = volume.data_ptr()
    return capacity


def tsdf_extract(volume: torch.Tensor, *, origin: Sequence[float], voxel_size: float, min_weight: int = 1, workspace: torch.Tensor,
                 records: Optional[torch.Tensor] = None, gradients: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None) -> None:
    """s2m2_tsdf_extract (K24): the surface points of ``volume`` (Nz,Ny,Nx,4) int32 -> the outputs the caller allocated: ``records``
    (capacity, 4) int32 = 16-byte records, ``gradients`` (capacity, 3) fp32, ``count`` (1) int32; ``records`` and ``gradients`` share one
    capacity; ``workspace``: ``tsdf_workspace_bytes`` bytes.  Thin: no allocation, no synchronisation."""
    _h._resident("tsdf_extract", volume, workspace, records, gradients, count)
    _h._contig("tsdf_extract", volume, workspace, records, gradients, count)
    d = _h.TsdfExtractDesc()
    capacity = _extract_operands("tsdf_extract", d, volume, origin, voxel_size, min_weight, records, gradients, count)
    if not capacity and count is None:
        raise ValueError("tsdf_extract: no output requested")
    need = tsdf_workspace_bytes(d.Nx, d.Ny, d.Nz)
    if workspace is None or workspace.nbytes < need:
        raise ValueError(f"tsdf_extract: a workspace of {need} bytes is required")
    d.workspace = workspace.data_ptr()
    with torch.cuda.device(volume.device):
        _h._check(_h.load().s2m2_tsdf_extract(ctypes.byref(d), _h._stream()), "s2m2_tsdf_extract")


def tsdf_mesh(volume: torch.Tensor, *, origin: Sequence[float], voxel_size: float, min_weight: int = 1, workspace: torch.Tensor,
              face_count: torch.Tensor, faces: Optional[torch.Tensor] = None, records: Optional[torch.Tensor] = None,
              gradients: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None) -> None:
    """s2m2_tsdf_mesh (K25): the surface of ``volume`` (Nz,Ny,Nx,4) int32 as a triangle mesh -> the outputs the caller allocated: ``faces``
    (face_capacity, 3) int32 vertex ranks and ``face_count`` (1) int32 (required: the true number of faces), plus ``tsdf_extract``'s
    ``records``, ``gradients`` and ``count`` (the vertices, each optional, byte-identical to ``tsdf_extract``'s); ``workspace``:
    ``tsdf_mesh_workspace_bytes`` bytes.  Thin: no allocation, no synchronisation."""
    _h._resident("tsdf_mesh", volume, workspace, face_count, faces, records, gradients, count)
    _h._contig("tsdf_mesh", volume, workspace, face_count, faces, records, gradients, count)
    d = _h.TsdfMeshDesc()
    _extract_operands("tsdf_mesh", d.extract, volume, origin, voxel_size, min_weight, records, gradients, count)
    if face_count is None:
        raise ValueError("tsdf_mesh: face_count is required")
    _h._vec(face_count, 1, "tsdf_mesh: face_count", dtype=torch.int32)
    d.face_count = face_count.data_ptr()
    if faces is not None:
        if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
            raise ValueError("tsdf_mesh: faces must be a (face_capacity, 3) int32 tensor")
        d.face_capacity = faces.shape[0]
        d.faces = _h._ptr(faces) if faces.shape[0] else None
    need = tsdf_mesh_workspace_bytes(d.extract.Nx, d.extract.Ny, d.extract.Nz)
    if workspace is None or workspace.nbytes < need:
        raise ValueError(f"tsdf_mesh: a workspace of {need} bytes is required")
    d.extract.workspace = workspace.data_ptr()
    with torch.cuda.device(volume.device):
        _h._check(_h.load().s2m2_tsdf_mesh(ctypes.byref(d), _h._stream()), "s2m2_tsdf_mesh")


RAYCAST_MAX_STEPS = 65536


def _f32(x: float) -> float:
    return ctypes.c_float(float(x)).value


def tsdf_raycast_steps(z_near: float, z_far: float, step: float) -> int:
    """the length of ``tsdf_raycast``'s march as the entry point computes it: ceil((z_far - z_near) / step) in double from the fp32 values;
    raises unless 0 <= z_near < z_far and step > 0 hold for the fp32 values and all three are finite"""
    zn, zf, st = _f32(z_near), _f32(z_far), _f32(step)                  # (a double beyond the fp32 range becomes inf)
    if not (math.isfinite(zn) and math.isfinite(zf) and math.isfinite(st) and 0.0 <= zn < zf and st > 0.0):
        raise ValueError(f"tsdf_raycast: finite 0 <= z_near < z_far and step > 0 are required in fp32, got z_near={z_near} z_far={z_far} step={step}")
    q = (zf - zn) / st
    return math.ceil(q) if q < 1e18 else 10 ** 18


def tsdf_raycast(volume: torch.Tensor, poses: torch.Tensor, *, Ht: int, Wt: int, fx: float, fy: float, cx: float, cy: float,
                 origin: Sequence[float], voxel_size: float, min_weight: int = 1, z_near: float = 0.0, z_far: float, step: float,
                 depth: Optional[torch.Tensor] = None, gradients: Optional[torch.Tensor] = None, image: Optional[torch.Tensor] = None,
                 count: Optional[torch.Tensor] = None) -> None:
    """s2m2_tsdf_raycast (K26): ``volume`` (Nz,Ny,Nx,4) int32 seen from the B cameras of the DEVICE pose buffer ``poses`` (B,12) fp32 ([R | t]
    row-major, world -> camera) with the intrinsics fx, fy, cx, cy and Ht x Wt pixels -> the outputs the caller allocated, each optional, at
    least one: ``depth`` (B,1,Ht,Wt) fp32 (0: hole), ``gradients`` (B,3,Ht,Wt) fp32 (world frame, unnormalised), ``image`` (B,3,Ht,Wt) uint8,
    ``count`` (B) int32 covered pixels.  The rays are sampled at z_near + k * step below z_far.  Thin: no allocation, no synchronisation."""
    _h._resident("tsdf_raycast", volume, poses, depth, gradients, image, count)
    _h._contig("tsdf_raycast", volume, poses, depth, gradients, image, count)
    d = _h.TsdfRaycastDesc()
    d.Nx, d.Ny, d.Nz = _volume("tsdf_raycast", volume)
    if poses is None or poses.dim() != 2 or poses.shape[0] < 1:
        raise ValueError("tsdf_raycast: poses must be a (B, 12) fp32 tensor with B >= 1")
    B = poses.shape[0]
    _h._mat(poses, (B, 12), torch.float32, "tsdf_raycast: poses")
    if int(Ht) != Ht or int(Wt) != Wt or Ht < 1 or Wt < 1 or B * int(Ht) * int(Wt) >= 1 << 31:
        raise ValueError(f"tsdf_raycast: bad extents B={B} Ht={Ht} Wt={Wt} (positive, B*Ht*Wt < 2^31)")
    Ht, Wt = int(Ht), int(Wt)
    if depth is None and gradients is None and image is None and count is None:
        raise ValueError("tsdf_raycast: no output requested")
    if depth is not None:
        _h._mat(depth, (B, 1, Ht, Wt), torch.float32, "tsdf_raycast: depth")
    if gradients is not None:
        _h._mat(gradients, (B, 3, Ht, Wt), torch.float32, "tsdf_raycast: gradients")
    if image is not None:
        _h._mat(image, (B, 3, Ht, Wt), torch.uint8, "tsdf_raycast: image")
    if count is not None:
        _h._vec(count, B, "tsdf_raycast: count", dtype=torch.int32)
    for name, x in (("fx", fx), ("fy", fy)):
        if not math.isfinite(float(x)) or abs(float(x)) > 3.4e38 or _f32(x) == 0.0:
            raise ValueError(f"tsdf_raycast: {name} must be finite and non-zero in fp32, got {x}")
    if not (math.isfinite(float(cx)) and math.isfinite(float(cy))):
        raise ValueError(f"tsdf_raycast: cx and cy must be finite, got {cx} and {cy}")
    d.origin, d.voxel_size = _placement("tsdf_raycast", origin, voxel_size)
    if int(min_weight) != min_weight or min_weight < 1:
        raise ValueError(f"tsdf_raycast: min_weight must be an integer >= 1, got {min_weight}")
    n_steps = tsdf_raycast_steps(z_near, z_far, step)
    if n_steps > RAYCAST_MAX_STEPS:
        raise ValueError(f"tsdf_raycast: {n_steps} steps from z_near={z_near} to z_far={z_far} (at most {RAYCAST_MAX_STEPS})")
    d.volume, d.poses = volume.data_ptr(), poses.data_ptr()
    d.depth, d.gradients, d.image, d.count = _h._ptr(depth), _h._ptr(gradients), _h._ptr(image), _h._ptr(count)
    d.B, d.Ht, d.Wt, d.min_weight = B, Ht, Wt, int(min_weight)
    d.fx, d.fy, d.cx, d.cy = float(fx), float(fy), float(cx), float(cy)
    d.z_near, d.z_far, d.step = float(z_near), float(z_far), float(step)
    with torch.cuda.device(volume.device):
        _h._check(_h.load().s2m2_tsdf_raycast(ctypes.byref(d), _h._stream()), "s2m2_tsdf_raycast")


TRACK_MAX_ITERS = 64


def _positive_f32(what: str, name: str, x: float) -> float:
    if not (math.isfinite(float(x)) and abs(float(x)) <= 3.4e38 and _f32(x) > 0.0):
        raise ValueError(f"{what}: {name} must be finite and > 0 in fp32, got {x}")
    return float(x)


def tsdf_track(disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, poses: torch.Tensor, model_poses: torch.Tensor,
               model_depth: torch.Tensor, model_gradients: torch.Tensor, *, H: int, W: int, fx: float, fy: float, cx: float, cy: float,
               baseline: float, doffs: float = 0.0, depth_scale: float = 1000.0, depth_trunc: float = 0.0, conf_min: float = 0.1,
               occ_min: float = 0.5, unfiltered: bool = False, mfx: float, mfy: float, mcx: float, mcy: float, max_dist: float,
               min_count: int = 6, max_rot: float, max_trans: float, n_iters: int, workspace: torch.Tensor,
               systems: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None) -> None:
    """s2m2_tsdf_track (K27): the live frame -- the B padded maps (B,1,Hp,Wp) fp32 with the fused crop H x W and K15's camera and filter
    numbers -- is registered to the model maps that ``tsdf_raycast`` rendered from ``model_poses`` (B,12) through the camera mfx, mfy, mcx,
    mcy: ``model_depth`` (B,1,Ht,Wt) and ``model_gradients`` (B,3,Ht,Wt) fp32.  ``poses`` (B,12) fp32 on the device ([R | t] row-major,
    world -> camera) holds the initial guess and is REFINED IN PLACE by ``n_iters`` point-to-plane iterations.  Optional outputs the caller
    allocated: ``systems`` (B, n_iters, 32) float64 and ``residual`` (B,1,H,W) fp32; ``workspace``: ``tsdf_track_workspace_bytes`` bytes.
    Thin: no allocation, no synchronisation."""
    what = "tsdf_track"
    _h._resident(what, disp, occ, conf, poses, model_poses, model_depth, model_gradients, workspace, systems, residual)
    _h._contig(what, disp, occ, conf, poses, model_poses, model_depth, model_gradients, workspace, systems, residual)
    d = _h.TsdfTrackDesc()
    if int(H) != H or int(W) != W:
        raise ValueError(f"{what}: H and W must be integers, got {H} and {W}")
    B, H, W = _h._cloud_inputs(what, d.cloud, disp, occ, conf, None, int(H), int(W), fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc,
                               conf_min, occ_min, unfiltered)
    if not (1 <= H <= disp.shape[2] and 1 <= W <= disp.shape[3]):
        raise ValueError(f"{what}: the crop H={H} W={W} must be positive and no larger than the maps {tuple(disp.shape[2:])}")
    for name, t in (("poses", poses), ("model_poses", model_poses)):
        if t is None:
            raise ValueError(f"{what}: {name} is required")
        _h._mat(t, (B, 12), torch.float32, f"{what}: {name}")
    if model_depth is None or model_depth.dim() != 4:
        raise ValueError(f"{what}: model_depth must be a (B,1,Ht,Wt) fp32 tensor")
    Ht, Wt = model_depth.shape[2:]
    if Ht < 1 or Wt < 1 or B * Ht * Wt >= 1 << 31:
        raise ValueError(f"{what}: bad model extents B={B} Ht={Ht} Wt={Wt} (positive, B*Ht*Wt < 2^31)")
    _h._mat(model_depth, (B, 1, Ht, Wt), torch.float32, f"{what}: model_depth")
    if model_gradients is None:
        raise ValueError(f"{what}: model_gradients is required")
    _h._mat(model_gradients, (B, 3, Ht, Wt), torch.float32, f"{what}: model_gradients")
    for name, x in (("mfx", mfx), ("mfy", mfy)):
        if not math.isfinite(float(x)) or abs(float(x)) > 3.4e38 or _f32(x) == 0.0:
            raise ValueError(f"{what}: {name} must be finite and non-zero in fp32, got {x}")
    if not (math.isfinite(float(mcx)) and math.isfinite(float(mcy))):
        raise ValueError(f"{what}: mcx and mcy must be finite, got {mcx} and {mcy}")
    d.max_dist = _positive_f32(what, "max_dist", max_dist)
    d.max_rot = _positive_f32(what, "max_rot", max_rot)
    d.max_trans = _positive_f32(what, "max_trans", max_trans)
    if int(min_count) != min_count or min_count < 6:
        raise ValueError(f"{what}: min_count must be an integer >= 6, got {min_count}")
    if int(n_iters) != n_iters or not 1 <= n_iters <= TRACK_MAX_ITERS:
        raise ValueError(f"{what}: n_iters must be an integer in 1..{TRACK_MAX_ITERS}, got {n_iters}")
    n_iters = int(n_iters)
    if systems is not None:
        _h._mat(systems, (B, n_iters, 32), torch.float64, f"{what}: systems")
    if residual is not None:
        _h._mat(residual, (B, 1, H, W), torch.float32, f"{what}: residual")
    need = tsdf_track_workspace_bytes(B, H, W)
    if workspace is None or workspace.nbytes < need or workspace.data_ptr() % 8:
        raise ValueError(f"{what}: an 8-byte aligned workspace of {need} bytes is required")
    d.poses, d.model_poses = poses.data_ptr(), model_poses.data_ptr()
    d.model_depth, d.model_gradients = model_depth.data_ptr(), model_gradients.data_ptr()
    d.systems, d.residual, d.workspace = _h._ptr(systems), _h._ptr(residual), workspace.data_ptr()
    d.Ht, d.Wt, d.min_count, d.n_iters = Ht, Wt, int(min_count), n_iters
    d.mfx, d.mfy, d.mcx, d.mcy = float(mfx), float(mfy), float(mcx), float(mcy)
    with torch.cuda.device(disp.device):
        _h._check(_h.load().s2m2_tsdf_track(ctypes.byref(d), _h._stream()), "s2m2_tsdf_track")


def tsdf_track_workspace_bytes(B: int, H: int, W: int) -> int:
    """bytes of ``tsdf_track``'s workspace: 32 doubles per tile (whole rows, as many as fit 4096 pixels) of the B live frames"""
    return _h._extent_query("s2m2_tsdf_track_workspace_bytes", "tsdf_track", B=B, H=H, W=W)


def tsdf_workspace_bytes(Nx: int, Ny: int, Nz: int) -> int:
    return _h._extent_query("s2m2_tsdf_workspace_bytes", "tsdf", Nx=Nx, Ny=Ny, Nz=Nz)


def tsdf_mesh_workspace_bytes(Nx: int, Ny: int, Nz: int) -> int:
    """bytes of ``tsdf_mesh``'s workspace: 4 per voxel and 8 per tile; refuses more than (2^31 - 1) / 5 voxels"""
    return _h._extent_query("s2m2_tsdf_mesh_workspace_bytes", "tsdf_mesh", Nx=Nx, Ny=Ny, Nz=Nz)


def tsdf_tile_voxels(Nx: int, Ny: int, Nz: int) -> int:
    """consecutive voxels of one tile of the extraction launches at these dims"""
    return _h._extent_query("s2m2_tsdf_tile_voxels", "tsdf", Nx=Nx, Ny=Ny, Nz=Nz)
