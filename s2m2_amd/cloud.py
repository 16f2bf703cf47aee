"""3D outputs behind ``S2M2.forward``: validity filter, metric depth and a coloured point cloud, on the device (K15, ``s2m2_cloud``).

The reference's demos do this on the host with numpy and open3d (demo/visualize_3d_middlebury.py:32-52,97-107,
src/s2m2/core/utils/model_utils.py:111-136, the mask of vis_utils.py:62).  Here ``reproject`` takes the padded maps as the forward returns them
and the unpadded left image, and leaves everything on the device: two kernel launches, no synchronisation, capturable in a hipGraph.  Between
its inputs and its outputs this module only allocates; the host reads ``count`` in ``PointCloud.points`` / ``colors`` / ``write_ply`` alone.

``mesh`` (K20, ``s2m2_mesh``) adds the surface: the same vertices plus the triangles that connect neighbouring kept pixels whose disparities
differ by at most ``max_jump``, as int32 vertex ranks in raster order of their quads (the rule: include/s2m2_hip.h, K20).  Three launches, no
synchronisation, capturable; the host reads the counts in the accessors of ``Mesh`` alone.

``register`` (K21, ``s2m2_register``) moves the depth map into another camera -- the colour camera of a rig, the right view (``right_camera``),
a virtual view: a z-buffered forward warp that keeps the nearest surface per target pixel, with the winners' colours, their source indices and
the visibility of every left pixel from that camera (the rule: include/s2m2_hip.h, K21).  Three launches, no synchronisation, capturable.

``segment`` (K22, ``s2m2_segment``) is the speckle filter in front of all three: the connected components of the kept pixels under ``mesh``'s
"joined" rule on the 4-neighbourhood, their sizes, and the disparity map with the components below ``min_size`` removed (the rule:
include/s2m2_hip.h, K22).  Four launches, no synchronisation, capturable.

``voxelize`` (K23, ``s2m2_voxel``) is the step every consumer of the cloud takes first: one point per occupied cell of a voxel grid, the centroid
and the mean colour of the kept points in it, in K15's record format and in the raster order of the cells' first points (the rule:
include/s2m2_hip.h, K23).  Four launches (five with the per-pixel index), no synchronisation, capturable, bit-reproducible.

``TsdfVolume`` (K24, ``s2m2_tsdf_integrate`` / ``s2m2_tsdf_extract``) is the first stage that carries state from one pair to the next: a dense
truncated signed distance volume on the device that ``integrate`` fuses the depth maps of a moving rig into, pose by pose, and whose surface
``extract`` returns as points with colours and gradients (the rule: include/s2m2_hip.h, K24).  One launch per call of ``integrate``, two per
``extract``, no synchronisation, capturable, bit-reproducible.  ``extract_mesh`` (K25, ``s2m2_tsdf_mesh``) returns that surface as a triangle
mesh: ``extract``'s points as vertices and the marching-cubes faces between them (the rule: include/s2m2_hip.h, K25).  Three launches.

``normals`` (K28, ``s2m2_normals``) gives the maps of ONE frame an orientation: the unit normal of every kept pixel in the camera frame, from
the neighbours ``radius`` pixels away (the rule: include/s2m2_hip.h, K28), as a ``NormalMap`` -- a ``TsdfRender`` with identity poses.  It fills
the normals of ``PointCloud.write_ply`` / ``Mesh.write_ply``, and ``track`` registers the next frame against it: K27 without a volume,
frame-to-frame odometry.  One launch, no synchronisation, capturable.

``smooth`` (K29, ``s2m2_smooth``) comes in front of all of them: an edge-preserving (bilateral) filter of the disparity map with a jump gate,
whose output has ``Segments.disp``'s form -- the padded map with -1 at dropped pixels, for any stage with ``filtered=False`` (the rule:
include/s2m2_hip.h, K29).  One launch, no synchronisation, capturable, bit-reproducible.

A record is 16 bytes --``float x, y, z; uint8 r, g, b, a`` (a = 255) -- which is the vertex of a binary little-endian PLY: ``write_ply_records``
writes a record buffer as it is.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import hip

PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n")
PLY_MESH_HEADER = PLY_HEADER.replace("end_header\n", "element face %d\nproperty list uchar int vertex_indices\nend_header\n")
FACE_DISK_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])        # 13 bytes per face on disk
RECORD_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
PLY_NORMALS_HEADER = PLY_HEADER.replace("property uchar red", "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red")
NORMAL_RECORD_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"),
                                ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
PLY_MESH_NORMALS_HEADER = PLY_NORMALS_HEADER.replace("end_header\n", "element face %d\nproperty list uchar int vertex_indices\nend_header\n")


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


def write_ply_mesh(path: str, records, faces, normals: bool = False) -> tuple:
    """Host function: n vertex records (as for ``write_ply_records``; with ``normals`` 28-byte ``NORMAL_RECORD_DTYPE`` records, nx ny nz
    between the position and the colour) and an (m,3) integer array of vertex indices -> binary little-endian PLY with ``element face m`` /
    ``property list uchar int vertex_indices``; returns (n, m)."""
    raw = records if isinstance(records, (bytes, bytearray)) else np.ascontiguousarray(records).tobytes()
    size = NORMAL_RECORD_DTYPE.itemsize if normals else 16
    if len(raw) % size:
        raise ValueError(f"write_ply_mesh: the vertex buffer is not a whole number of {size}-byte records")
    faces = np.asarray(faces)
    if faces.size == 0:
        faces = faces.reshape(0, 3)
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype.kind not in "iu":
        raise ValueError("write_ply_mesh: faces must be an (m,3) integer array")
    n, m = len(raw) // size, faces.shape[0]
    if m and (int(faces.min()) < 0 or int(faces.max()) >= n):
        raise ValueError(f"write_ply_mesh: a face references a vertex outside 0..{n - 1}")
    disk = np.empty(m, dtype=FACE_DISK_DTYPE)
    disk["n"], disk["v"] = 3, faces
    with open(path, "wb") as f:
        f.write(((PLY_MESH_NORMALS_HEADER if normals else PLY_MESH_HEADER) % (n, m)).encode("ascii"))
        f.write(raw)
        f.write(disk.tobytes())
    return n, m


def read_ply_mesh(path: str) -> tuple:
    """The inverse of ``write_ply_mesh`` for files with exactly its layouts -> (``RECORD_DTYPE`` array, or ``NORMAL_RECORD_DTYPE`` for a
    file with normals, (m,3) int32 array)."""
    raw = open(path, "rb").read()
    end = raw.find(b"end_header\n")
    if not raw.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    head = raw[:end + len(b"end_header\n")].decode("ascii")
    counts = [int(line.split()[2]) for line in head.split("\n") if line.startswith("element")]
    layouts = [(h, t) for h, t in ((PLY_MESH_HEADER, RECORD_DTYPE), (PLY_MESH_NORMALS_HEADER, NORMAL_RECORD_DTYPE))
               if len(counts) == 2 and head == h % tuple(counts)]
    if not layouts:
        raise ValueError(f"{path}: not the vertex + triangle layout of write_ply_mesh")
    n, m = counts
    vertex = layouts[0][1]
    body = raw[len(head):]
    if len(body) != vertex.itemsize * n + 13 * m:
        raise ValueError(f"{path}: {n} vertices and {m} faces declared, {len(body)} bytes of data")
    disk = np.frombuffer(body, dtype=FACE_DISK_DTYPE, offset=vertex.itemsize * n)
    if m and not (disk["n"] == 3).all():
        raise ValueError(f"{path}: a face is not a triangle")
    return np.frombuffer(body, dtype=vertex, count=n), np.ascontiguousarray(disk["v"])


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

    def _normal_records(self, b: int, normals: "NormalMap", what: str) -> np.ndarray:
        """the stored records of pair b with the normals of ``normals`` -- a ``NormalMap`` of the same maps, camera and filter keywords, whose
        kept pixels (depth > 0) in raster order are this cloud's records in record order -- as a ``NORMAL_RECORD_DTYPE`` array; a kept pixel
        without a normal gets 0,0,0"""
        n = int(self.count[b].item())
        if n > self.capacity:
            raise ValueError(f"{what}: pair {b} has {n} points but a capacity of {self.capacity}: the normals of the unstored points have no record")
        kept = normals.depth[b, 0] > 0
        nrm = normals.gradients_buf[b][:, kept].t().cpu().numpy()
        if len(nrm) != n:
            raise ValueError(f"{what}: the normal map keeps {len(nrm)} pixels of pair {b}, the cloud {n}: not the same maps, camera or filter")
        rec = self.records[b, :n].cpu().numpy().view(RECORD_DTYPE).ravel()
        out = np.empty(n, dtype=NORMAL_RECORD_DTYPE)
        for name in RECORD_DTYPE.names:
            out[name] = rec[name]
        out["nx"], out["ny"], out["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
        return out

    def write_ply(self, path: str, b: int = 0, normals: Optional["NormalMap"] = None) -> int:
        """the stored records of pair b as a binary PLY; ``normals``: a ``NormalMap`` computed with the same camera and filter keywords adds
        nx, ny, nz per vertex between the position and the colour (raises when its kept pixels are not this cloud's points)"""
        if normals is None:
            return write_ply_records(path, self.records[b, :self.size(b)].cpu().numpy())
        out = self._normal_records(b, normals, "PointCloud.write_ply")
        with open(path, "wb") as f:
            f.write((PLY_NORMALS_HEADER % len(out)).encode("ascii"))
            f.write(out.tobytes())
        return len(out)


def _binding_kwargs(fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min, occ_min, filtered) -> Dict[str, object]:
    """``reproject``'s conventions -> the camera and filter keywords of the binding (hip.cloud, hip.mesh, hip.register, hip.segment): fy
    defaults to fx and depth_trunc None is 1e9, both as in the reference; filtered becomes unfiltered; the rest passes through."""
    return dict(fx=fx, fy=fx if fy is None else fy, cx=cx, cy=cy, baseline=baseline, doffs=doffs, depth_scale=depth_scale,
                depth_trunc=1e9 if depth_trunc is None else depth_trunc, conf_min=conf_min, occ_min=occ_min, unfiltered=not filtered)


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
    hip.cloud(disp, occ, conf, image, **_binding_kwargs(fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min, occ_min, filtered),
              records=records, count=count, workspace=workspace, depth=depth, mask=mask)
    return PointCloud(records, count, depth, mask)


class Mesh(PointCloud):
    """What ``mesh`` returns: a ``PointCloud`` (the vertices) plus ``faces_buf`` (B, face_capacity, 3) int32 vertex ranks in raster order of
    their quads, ``face_count`` (B) int32 on the device (the true number of faces, also above face_capacity) and the optional dense rank map
    ``index`` (B,1,H,W) int32 (-1: not a vertex)."""

    def __init__(self, records: torch.Tensor, count: torch.Tensor, faces_buf: torch.Tensor, face_count: torch.Tensor,
                 index: Optional[torch.Tensor] = None, depth: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None):
        super().__init__(records, count, depth, mask)
        self.faces_buf, self.face_count, self.index = faces_buf, face_count, index

    @property
    def face_capacity(self) -> int:
        return self.faces_buf.shape[1]

    def face_size(self, b: int = 0) -> int:
        """faces stored for pair b: min(face_count, face_capacity) -- reads ``face_count`` on the host (synchronises)"""
        return min(int(self.face_count[b].item()), self.face_capacity)

    def faces(self, b: int = 0) -> torch.Tensor:
        """(n,3) int32 view of the stored faces of pair b.  Raises when the vertices overflowed: the faces hold true ranks and would reference
        vertices that were not stored."""
        n = int(self.count[b].item())
        if n > self.capacity:
            raise ValueError(f"Mesh.faces: pair {b} has {n} vertices but a capacity of {self.capacity}: the faces reference unstored vertices")
        return self.faces_buf[b, :self.face_size(b)]

    def write_ply(self, path: str, b: int = 0, normals: Optional["NormalMap"] = None) -> tuple:
        """vertices and faces of pair b in ``write_ply_mesh``'s layout; ``normals``: as for ``PointCloud.write_ply``"""
        faces = self.faces(b).cpu().numpy()
        if normals is None:
            return write_ply_mesh(path, self.records[b, :self.size(b)].cpu().numpy(), faces)
        return write_ply_mesh(path, self._normal_records(b, normals, "Mesh.write_ply"), faces, normals=True)


def mesh(disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, image: torch.Tensor, *, fx: float, cx: float, cy: float, baseline: float,
         doffs: float = 0.0, fy: Optional[float] = None, depth_scale: float = 1000.0, depth_trunc: Optional[float] = None,
         conf_min: float = 0.1, occ_min: float = 0.5, filtered: bool = True, max_jump: float = 1.0, capacity: Optional[int] = None,
         face_capacity: Optional[int] = None, want_depth: bool = False, want_mask: bool = False, want_index: bool = False) -> Mesh:
    """``reproject``'s operands and conventions -> Mesh.  Neighbouring kept pixels are connected where their disparities differ by at most
    ``max_jump`` (full-resolution pixels; inf connects every kept neighbour).  capacity None = H*W vertices, face_capacity None =
    2*(H-1)*(W-1) faces per pair: nothing can overflow."""
    B = disp.shape[0]
    H, W = image.shape[-2:]
    cap = H * W if capacity is None else int(capacity)
    fcap = 2 * (H - 1) * (W - 1) if face_capacity is None else int(face_capacity)
    if cap < 0 or fcap < 0:
        raise ValueError("mesh: negative capacity")
    dev = disp.device
    records = torch.empty((B, cap, 4), device=dev, dtype=torch.int32)
    count = torch.empty((B,), device=dev, dtype=torch.int32)
    faces = torch.empty((B, fcap, 3), device=dev, dtype=torch.int32)
    face_count = torch.empty((B,), device=dev, dtype=torch.int32)
    workspace = torch.empty((hip.mesh_workspace_bytes(B, H, W),), device=dev, dtype=torch.uint8)
    index = torch.empty((B, 1, H, W), device=dev, dtype=torch.int32) if want_index else None
    depth = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32) if want_depth else None
    mask = torch.empty((B, 1, H, W), device=dev, dtype=torch.uint8) if want_mask else None
    hip.mesh(disp, occ, conf, image, **_binding_kwargs(fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min, occ_min, filtered),
             max_jump=max_jump, records=records, count=count, faces=faces, face_count=face_count, workspace=workspace, index=index, depth=depth,
             mask=mask)
    return Mesh(records, count, faces, face_count, index, depth, mask)


class Camera:
    """A pinhole target camera for ``register``: the image size, the intrinsics and the pose relative to the rectified left camera -- a point p
    of the left camera's frame is ``R @ p + t`` in this camera's (``R`` (3,3), ``t`` (3,) in the unit of z, i.e. after ``depth_scale``)."""

    def __init__(self, width: int, height: int, fx: float, fy: float, cx: float, cy: float, R=None, t=None):
        self.width, self.height = int(width), int(height)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3)
        self.t = np.zeros(3) if t is None else np.asarray(t, dtype=np.float64).reshape(3)

    def __repr__(self) -> str:
        return (f"Camera({self.width}x{self.height}, fx={self.fx}, fy={self.fy}, cx={self.cx}, cy={self.cy}, R={self.R.tolist()}, "
                f"t={self.t.tolist()})")


def right_camera(calib: Dict[str, object], width: int, height: int, depth_scale: float = 1000.0) -> Camera:
    """The rectified right view of a Middlebury calib (``read_calib_file``): cam1's intrinsics, no rotation, and the left camera's origin
    one baseline to the left of the right camera's: t = (-baseline / depth_scale, 0, 0)."""
    k = np.asarray(calib["cam1"], dtype=np.float64)
    return Camera(width, height, k[0, 0], k[1, 1], k[0, 2], k[1, 2], np.eye(3), (-float(calib["baseline"]) / float(depth_scale), 0.0, 0.0))


class Registered:
    """What ``register`` returns, all on the device and in the TARGET camera unless noted: ``depth`` (B,1,Ht,Wt) fp32 z of the nearest surface
    (0: hole), ``index`` (B,1,Ht,Wt) int32 source pixel v*W+u that won (-1: hole), ``image`` (B,3,Ht,Wt) uint8 or None, ``visible`` (B,1,H,W)
    uint8 in the SOURCE camera (1: the pixel won a target pixel) or None, ``count`` (B) int32 covered target pixels or None."""

    def __init__(self, depth: torch.Tensor, index: torch.Tensor, image: Optional[torch.Tensor], visible: Optional[torch.Tensor],
                 count: Optional[torch.Tensor]):
        self.depth, self.index, self.image, self.visible, self.count = depth, index, image, visible, count

    def holes(self, b: int = 0) -> int:
        """target pixels of pair b that nothing covers -- reads ``count`` on the host (synchronises)"""
        if self.count is None:
            raise ValueError("Registered.holes: register was called with want_count=False")
        return self.depth.shape[-2] * self.depth.shape[-1] - int(self.count[b].item())


def register(disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, image: torch.Tensor, *, fx: float, cx: float, cy: float, baseline: float,
             doffs: float = 0.0, to: Camera, splat: int = 2, fy: Optional[float] = None, depth_scale: float = 1000.0,
             depth_trunc: Optional[float] = None, conf_min: float = 0.1, occ_min: float = 0.5, filtered: bool = True, want_image: bool = True,
             want_visible: bool = False, want_count: bool = True) -> Registered:
    """``reproject``'s operands and conventions -> the depth map in the camera ``to`` (K21, ``s2m2_register``): every kept pixel is
    back-projected as in ``reproject``, moved by ``to.R``, ``to.t``, projected and splatted over ``splat`` x ``splat`` target pixels into a
    z-buffer that keeps the nearest surface (the rule: include/s2m2_hip.h, K21).  Three launches, no synchronisation, capturable."""
    B = disp.shape[0]
    H, W = image.shape[-2:]
    Ht, Wt = to.height, to.width
    dev = disp.device
    depth = torch.empty((B, 1, Ht, Wt), device=dev, dtype=torch.float32)
    index = torch.empty((B, 1, Ht, Wt), device=dev, dtype=torch.int32)
    image_t = torch.empty((B, 3, Ht, Wt), device=dev, dtype=torch.uint8) if want_image else None
    visible = torch.empty((B, 1, H, W), device=dev, dtype=torch.uint8) if want_visible else None
    count = torch.empty((B,), device=dev, dtype=torch.int32) if want_count else None
    workspace = torch.empty((hip.register_workspace_bytes(B, Ht, Wt),), device=dev, dtype=torch.uint8)
    hip.register(disp, occ, conf, image, **_binding_kwargs(fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min, occ_min, filtered),
                 Ht=Ht, Wt=Wt, splat=splat, fx_t=to.fx, fy_t=to.fy, cx_t=to.cx, cy_t=to.cy, R=to.R.ravel().tolist(), t=to.t.tolist(),
                 workspace=workspace, depth_t=depth, index_t=index, image_t=image_t, visible=visible, count=count)
    return Registered(depth, index, image_t, visible, count)


class Segments:
    """What ``segment`` returns, all on the device: ``disp`` (B,1,Hp,Wp) fp32, the PADDED disparity with -1 wherever the pixel does not survive
    (border included); ``mask`` (B,1,H,W) uint8 (1: kept and in a component of at least ``min_size`` pixels); ``label`` (B,1,H,W) int32 or None
    (raster index of the first pixel of the component, -1: not kept); ``size`` (B,1,H,W) int32 or None (pixels of the component, 0: not kept);
    ``stats`` (B,4) int32: kept pixels, components, surviving pixels, surviving components."""

    def __init__(self, disp: torch.Tensor, mask: torch.Tensor, label: Optional[torch.Tensor], size: Optional[torch.Tensor], stats: torch.Tensor):
        self.disp, self.mask, self.label, self.size, self.stats = disp, mask, label, size, stats

    def kept(self, b: int = 0) -> int:
        """kept pixels of pair b -- this and the three readers below read ``stats`` on the host (synchronise)"""
        return int(self.stats[b, 0].item())

    def components(self, b: int = 0) -> int:
        return int(self.stats[b, 1].item())

    def surviving(self, b: int = 0) -> int:
        return int(self.stats[b, 2].item())

    def surviving_components(self, b: int = 0) -> int:
        return int(self.stats[b, 3].item())


def segment(disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, *, H: int, W: int, fx: float, cx: float, cy: float, baseline: float,
            doffs: float = 0.0, fy: Optional[float] = None, depth_scale: float = 1000.0, depth_trunc: Optional[float] = None,
            conf_min: float = 0.1, occ_min: float = 0.5, filtered: bool = True, max_jump: float = 1.0, min_size: int = 1,
            want_label: bool = True, want_size: bool = True) -> Segments:
    """``reproject``'s maps and conventions (no image: ``H`` and ``W`` name the fused crop) -> Segments (K22, ``s2m2_segment``).  Kept
    neighbours in a row or a column are joined where their disparities differ by at most ``max_jump`` (``mesh``'s rule; inf joins every kept
    neighbour); a component is a class of the transitive closure; a pixel survives if it is kept and its component has at least ``min_size``
    pixels (1: nothing is removed).  Only allocates: four launches, no synchronisation, capturable.

    Composition: ``s = segment(...)`` then ``reproject(s.disp, occ, conf, image, ..., filtered=False)`` (or ``mesh`` / ``register``) gives
    exactly the surviving pixels with their original z -- whenever K15 itself drops d <= 0, that is whenever ``1e9 / depth_scale >=
    depth_trunc``.  With ``depth_trunc=None`` K15 keeps d <= 0 at z = 1e6 (depth_scale 1000) as the reference's formula does, the removed pixels
    included: pass a real truncation distance to the stage behind."""
    B, _, Hp, Wp = disp.shape
    dev = disp.device
    out = torch.empty((B, 1, Hp, Wp), device=dev, dtype=torch.float32)
    mask = torch.empty((B, 1, H, W), device=dev, dtype=torch.uint8)
    label = torch.empty((B, 1, H, W), device=dev, dtype=torch.int32) if want_label else None
    size = torch.empty((B, 1, H, W), device=dev, dtype=torch.int32) if want_size else None
    stats = torch.empty((B, 4), device=dev, dtype=torch.int32)
    workspace = torch.empty((hip.segment_workspace_bytes(B, H, W),), device=dev, dtype=torch.uint8)
    hip.segment(disp, occ, conf, H=H, W=W, **_binding_kwargs(fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min, occ_min, filtered),
                max_jump=max_jump, min_size=min_size, workspace=workspace, label=label, size=size, mask=mask,
                disp_out=out, stats=stats)
    return Segments(out, mask, label, size, stats)


class VoxelCloud(PointCloud):
    """What ``voxelize`` returns: a ``PointCloud`` whose records are voxels -- ``records`` (B, capacity, 4) int32 in the raster order of the
    voxels' first points, ``count`` (B) int32 (the true number of voxels, also above capacity) -- plus ``weights_buf`` (B, capacity) int32 or
    None (points per voxel), ``index`` (B,1,H,W) int32 or None (the record rank of every pixel's voxel, -1: not kept or dropped) and ``stats``
    (B,4) int32: kept points, points dropped out of range, points dropped because the table was full, voxels."""

    def __init__(self, records: torch.Tensor, count: torch.Tensor, weights_buf: Optional[torch.Tensor], index: Optional[torch.Tensor],
                 stats: torch.Tensor):
        super().__init__(records, count)
        self.weights_buf, self.index, self.stats = weights_buf, index, stats

    def weights(self, b: int = 0) -> torch.Tensor:
        """(n) int32: the points of every stored voxel of pair b"""
        if self.weights_buf is None:
            raise ValueError("VoxelCloud.weights: voxelize was called with want_weights=False")
        return self.weights_buf[b, :self.size(b)]

    def complete(self, b: int = 0) -> bool:
        """no point of pair b was dropped because the table was full -- reads ``stats`` on the host (synchronises).  False: the records of
        this pair are unspecified; call again with a larger ``max_voxels``"""
        return int(self.stats[b, 2].item()) == 0


def voxelize(disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, image: torch.Tensor, *, fx: float, cx: float, cy: float,
             baseline: float, doffs: float = 0.0, voxel_size: float, max_voxels: Optional[int] = None, capacity: Optional[int] = None,
             fy: Optional[float] = None, depth_scale: float = 1000.0, depth_trunc: Optional[float] = None, conf_min: float = 0.1,
             occ_min: float = 0.5, filtered: bool = True, want_weights: bool = True, want_index: bool = False) -> VoxelCloud:
    """``reproject``'s operands and conventions -> VoxelCloud (K23, ``s2m2_voxel``): the kept points fall into the cells of a grid of
    ``voxel_size`` (the unit of z) anchored at the camera origin, and every occupied cell gives one record: the centroid and the mean colour.
    Points beyond 2^20 cells from the origin on any axis are dropped and counted (``stats[:, 1]``): with ``depth_trunc=None`` those are the
    d <= 0 pixels K15 keeps at z = 1e9 / depth_scale.  Only allocates: no synchronisation, capturable.

    ``max_voxels`` (distinct voxels a pair may have) and ``capacity`` (records stored per pair) default to H*W // 4.  Memory: the hash table
    takes 64 bytes per slot and has 2 * max_voxels slots rounded up to a power of two -- 32 to 64 bytes per PIXEL at the default, 64 MiB at
    1216x1024 --, the slot plane 4 bytes per pixel, records and weights 20 bytes per unit of capacity.  A pair with more voxels than
    ``max_voxels`` drops points: ``complete(b)`` tells.

    Composition with K22: ``s = segment(...)`` then ``voxelize(s.disp, occ, conf, image, ..., filtered=False)`` downsamples exactly the
    surviving pixels (pass a real ``depth_trunc``, as for ``reproject`` behind ``segment``)."""
    B = disp.shape[0]
    H, W = image.shape[-2:]
    mv = max(1, H * W // 4) if max_voxels is None else max_voxels
    cap = max(1, H * W // 4) if capacity is None else int(capacity)
    if cap < 0:
        raise ValueError("voxelize: negative capacity")
    if int(mv) != mv or not 1 <= mv <= 1 << 29:
        raise ValueError(f"voxelize: max_voxels must be an integer in 1..2^29, got {max_voxels}")
    mv = int(mv)
    dev = disp.device
    workspace = torch.empty((hip.voxel_workspace_bytes(B, H, W, mv),), device=dev, dtype=torch.uint8)
    records = torch.empty((B, cap, 4), device=dev, dtype=torch.int32)
    count = torch.empty((B,), device=dev, dtype=torch.int32)
    weights = torch.empty((B, cap), device=dev, dtype=torch.int32) if want_weights else None
    index = torch.empty((B, 1, H, W), device=dev, dtype=torch.int32) if want_index else None
    stats = torch.empty((B, 4), device=dev, dtype=torch.int32)
    hip.voxel(disp, occ, conf, image, **_binding_kwargs(fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min, occ_min, filtered),
              voxel_size=voxel_size, max_voxels=mv, workspace=workspace, records=records, weights=weights, count=count, index=index, stats=stats)
    return VoxelCloud(records, count, weights, index, stats)


class TsdfSurface(PointCloud):
    """What ``TsdfVolume.extract`` returns: a ``PointCloud`` with one pair (b = 0) whose records are the surface points of the volume in
    ascending voxel order -- ``records`` (1, capacity, 4) int32, ``count`` (1) int32 (the true number of points, also above capacity) -- plus
    ``gradients_buf`` (capacity, 3) fp32 or None: the unnormalised tsdf gradient at every point, from the surface to free space."""

    def __init__(self, records: torch.Tensor, count: torch.Tensor, gradients_buf: Optional[torch.Tensor]):
        super().__init__(records, count)
        self.gradients_buf = gradients_buf

    def gradients(self) -> torch.Tensor:
        """(n,3) fp32: the tsdf gradient at every stored point"""
        if self.gradients_buf is None:
            raise ValueError("TsdfSurface.gradients: extract was called with want_gradients=False")
        return self.gradients_buf[:self.size()]

    def normals(self) -> torch.Tensor:
        """(n,3) fp32: the gradients normalised in torch (a zero gradient stays zero); not part of the exact contract"""
        g = self.gradients()
        return g / g.norm(dim=1, keepdim=True).clamp_min(1e-30)

    def write_ply(self, path: str, b: int = 0, normals: bool = False) -> int:
        if not normals:
            return super().write_ply(path, b)
        rec = self.records[0, :self.size()].cpu().numpy().view(RECORD_DTYPE).ravel()
        out = np.empty(len(rec), dtype=NORMAL_RECORD_DTYPE)
        for name in RECORD_DTYPE.names:
            out[name] = rec[name]
        nrm = self.normals().cpu().numpy()
        out["nx"], out["ny"], out["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
        with open(path, "wb") as f:
            f.write((PLY_NORMALS_HEADER % len(out)).encode("ascii"))
            f.write(out.tobytes())
        return len(out)


class TsdfMesh(TsdfSurface):
    """What ``TsdfVolume.extract_mesh`` returns: a ``TsdfSurface`` (the vertices: exactly ``extract``'s points) plus ``faces_buf``
    (face_capacity, 3) int32 vertex ranks, in ascending order of their cells and wound so that the normals point to free space, and
    ``face_count`` (1) int32 on the device (the true number of faces, also above face_capacity)."""

    def __init__(self, records: torch.Tensor, count: torch.Tensor, gradients_buf: Optional[torch.Tensor], faces_buf: torch.Tensor,
                 face_count: torch.Tensor):
        super().__init__(records, count, gradients_buf)
        self.faces_buf, self.face_count = faces_buf, face_count

    def face_capacity(self) -> int:
        return self.faces_buf.shape[0]

    def face_size(self) -> int:
        """faces stored: min(face_count, face_capacity) -- reads ``face_count`` on the host (synchronises)"""
        return min(int(self.face_count.item()), self.face_capacity())

    def faces(self) -> torch.Tensor:
        """(n,3) int32 view of the stored faces.  Raises when the vertices overflowed: the faces hold true ranks and would reference vertices
        that were not stored."""
        n = int(self.count[0].item())
        if n > self.capacity:
            raise ValueError(f"TsdfMesh.faces: {n} vertices but a capacity of {self.capacity}: the faces reference unstored vertices")
        return self.faces_buf[:self.face_size()]

    def write_ply(self, path: str, normals: bool = False) -> tuple:
        """vertices and faces in ``write_ply_mesh``'s layout -> (vertices, faces) written; ``normals``: nx, ny, nz per vertex from the
        normalised gradients, between the position and the colour"""
        faces = self.faces().cpu().numpy()
        rec = self.records[0, :self.size()].cpu().numpy()
        if not normals:
            return write_ply_mesh(path, rec, faces)
        rec = rec.view(RECORD_DTYPE).ravel()
        out = np.empty(len(rec), dtype=NORMAL_RECORD_DTYPE)
        for name in RECORD_DTYPE.names:
            out[name] = rec[name]
        nrm = self.normals().cpu().numpy()
        out["nx"], out["ny"], out["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
        return write_ply_mesh(path, out, faces, normals=True)


class TsdfRender:
    """What ``TsdfVolume.raycast`` returns, all on the device and in the target camera unless noted: ``depth`` (B,1,Ht,Wt) fp32 z of the first
    surface along the ray (0: hole), ``gradients_buf`` (B,3,Ht,Wt) fp32 or None: the unnormalised tsdf gradient at the hit in the WORLD frame,
    from the surface to free space (0 at holes), ``image`` (B,3,Ht,Wt) uint8 or None, ``count`` (B) int32 covered pixels or None; ``R``
    (B,3,3) fp32: the rotations the maps were rendered with.  ``raycast`` also sets ``poses`` (B,12) fp32, the device pose buffer of the render,
    and ``camera``, its ``Camera``: what ``TsdfVolume.track`` needs of the model side (None in a render built by hand without them)."""

    def __init__(self, depth: torch.Tensor, gradients_buf: Optional[torch.Tensor], image: Optional[torch.Tensor], count: Optional[torch.Tensor],
                 R: torch.Tensor, poses: Optional[torch.Tensor] = None, camera: Optional[Camera] = None):
        self.depth, self.gradients_buf, self.image, self.count, self.R = depth, gradients_buf, image, count, R
        self.poses, self.camera = poses, camera

    def normals(self) -> torch.Tensor:
        """(B,3,Ht,Wt) fp32 in the CAMERA frame: ``R @ G`` normalised in torch (a zero gradient stays zero); not part of the exact contract"""
        if self.gradients_buf is None:
            raise ValueError("TsdfRender.normals: raycast was called with want_gradients=False")
        g = torch.einsum("bij,bjhw->bihw", self.R.to(self.gradients_buf.device), self.gradients_buf)
        return g / g.norm(dim=1, keepdim=True).clamp_min(1e-30)

    def holes(self, b: int = 0) -> int:
        """pixels of pair b that no surface covers -- reads ``count`` on the host (synchronises)"""
        if self.count is None:
            raise ValueError("TsdfRender.holes: raycast was called with want_count=False")
        return self.depth.shape[-2] * self.depth.shape[-1] - int(self.count[b].item())


class TsdfTrack:
    """What ``TsdfVolume.track`` returns, all on the device: ``poses`` (B,12) fp32, the refined [R | t] per pair (world -> camera; the buffer
    that was passed in, where one was); ``R`` (B,3,3) and ``t`` (B,3): strided views of it; ``systems`` (B, n_iters, 32) float64 or None: per
    iteration the normal equations (A's upper triangle, sum J r, sum r^2), the count of correspondences, the status (0 accepted, 1 too few
    correspondences, 2 singular or non-finite, 3 step too long) and the norms of the step; ``residual`` (B,1,H,W) fp32 or None: the
    point-to-plane distance of the last iteration's correspondences, NaN elsewhere."""

    def __init__(self, poses: torch.Tensor, systems: Optional[torch.Tensor], residual: Optional[torch.Tensor]):
        self.poses, self.systems, self.residual = poses, systems, residual
        P = poses.view(poses.shape[0], 3, 4)
        self.R, self.t = P[:, :, :3], P[:, :, 3]

    def _last(self, b: int) -> torch.Tensor:
        if self.systems is None:
            raise ValueError("TsdfTrack: track was called with want_systems=False")
        return self.systems[b, -1].cpu()

    def status(self, b: int = 0) -> int:
        """the status of pair b's last iteration -- reads ``systems`` on the host (synchronises), like the three below"""
        return int(self._last(b)[29])

    def count(self, b: int = 0) -> int:
        """correspondences of the last iteration"""
        return int(self._last(b)[28])

    def rmse(self, b: int = 0) -> float:
        """sqrt(sum r^2 / count) of the last iteration (NaN without a correspondence)"""
        row = self._last(b)
        return float((row[27] / row[28]).sqrt()) if row[28] > 0 else float("nan")

    def ok(self, b: int = 0) -> bool:
        return self.status(b) == 0


class TsdfVolume:
    """A truncated signed distance volume on the device (K24, ``s2m2_tsdf_integrate`` / ``s2m2_tsdf_extract``; the rule: include/s2m2_hip.h,
    K24): ``dims`` = (Nx, Ny, Nz) voxels of ``voxel_size`` (the unit of z), ``origin`` the centre of voxel (0,0,0) in the world frame,
    ``trunc`` the truncation distance (None: 4 * voxel_size), ``max_weight`` the cap of a voxel's frame count.  ``buffer`` is the
    (Nz, Ny, Nx, 4) int32 tensor the kernels work on, 16 bytes per voxel; all zero = empty."""

    def __init__(self, dims, voxel_size: float, origin, trunc: Optional[float] = None, max_weight: int = 64, device="cuda"):
        Nx, Ny, Nz = (int(n) for n in dims)
        if min(Nx, Ny, Nz) < 1 or Nx * Ny * Nz >= 1 << 29:
            raise ValueError(f"TsdfVolume: bad dims {tuple(dims)} (positive, Nx*Ny*Nz < 2^29)")
        if not (np.isfinite(float(voxel_size)) and voxel_size > 0):
            raise ValueError(f"TsdfVolume: voxel_size must be finite and > 0, got {voxel_size}")
        trunc = 4.0 * float(voxel_size) if trunc is None else float(trunc)
        if not (np.isfinite(trunc) and trunc > 0):
            raise ValueError(f"TsdfVolume: trunc must be finite and > 0, got {trunc}")
        if int(max_weight) != max_weight or not 1 <= max_weight <= 32767:
            raise ValueError(f"TsdfVolume: max_weight must be an integer in 1..32767, got {max_weight}")
        self.dims, self.voxel_size, self.trunc, self.max_weight = (Nx, Ny, Nz), float(voxel_size), trunc, int(max_weight)
        self.origin = tuple(float(x) for x in origin)
        if len(self.origin) != 3 or not all(np.isfinite(self.origin)):
            raise ValueError("TsdfVolume: origin is three finite numbers")
        self.device = torch.device(device)
        self.buffer = torch.zeros((Nz, Ny, Nx, 4), device=self.device, dtype=torch.int32)
        self._workspace = None
        self._mesh_workspace = None
        self._track_workspace = None

    def reset(self) -> None:
        self.buffer.zero_()

    def tsdf(self) -> torch.Tensor:
        """(Nz, Ny, Nx) fp32 strided view"""
        return self.buffer.view(torch.float32)[..., 0]

    def weight(self) -> torch.Tensor:
        """(Nz, Ny, Nx) int32 strided view"""
        return self.buffer[..., 1]

    def colour(self) -> torch.Tensor:
        """(Nz, Ny, Nx, 3) int16 strided view of the 8.8 fixed-point r, g, b (read them as unsigned: value & 0xffff)"""
        return self.buffer.view(torch.int16)[..., 4:7]

    def _poses(self, R, t, B: int, what: str = "integrate") -> torch.Tensor:
        """R (3,3) or (B,3,3), t (3,) or (B,3), tensors on any device or anything ``torch.as_tensor`` takes -> (B,12) fp32 on the device"""
        R = torch.as_tensor(R).to(device=self.device, dtype=torch.float32)
        t = torch.as_tensor(t).to(device=self.device, dtype=torch.float32)
        if tuple(R.shape) not in ((3, 3), (B, 3, 3)) or tuple(t.shape) not in ((3,), (B, 3)):
            raise ValueError(f"TsdfVolume.{what}: R is (3,3) or ({B},3,3) and t is (3,) or ({B},3), got {tuple(R.shape)} and {tuple(t.shape)}")
        R = R.expand(B, 3, 3) if R.dim() == 2 else R
        t = t.expand(B, 3) if t.dim() == 1 else t
        return torch.cat([R, t[:, :, None]], dim=2).reshape(B, 12).contiguous()

    def integrate(self, disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, left_u8: torch.Tensor, *, R=None, t=None, fx: float,
                  cx: float, cy: float, baseline: float, doffs: float = 0.0, fy: Optional[float] = None, depth_scale: float = 1000.0,
                  depth_trunc: Optional[float] = None, conf_min: float = 0.1, occ_min: float = 0.5, filtered: bool = True,
                  carve: bool = False, poses: Optional[torch.Tensor] = None) -> "TsdfVolume":
        """``reproject``'s operands and conventions plus the pose of every pair (``p_cam = R @ p_world + t``, ``t`` in the unit of z): the B
        depth maps are fused into the volume in the order of the batch.  ``carve``: also the voxels between the camera and the band take the
        free-space value 1.  Instead of ``R`` and ``t``, ``poses`` takes a device (B,12) fp32 buffer as it is (``TsdfTrack.poses``: a tracked
        pose feeds the fusion without a copy).  One launch, no synchronisation, capturable; composes with ``segment(...).disp`` via
        ``filtered=False``."""
        if (poses is None) == (R is None or t is None):
            raise ValueError("TsdfVolume.integrate: pass the poses either as R and t or as poses")
        if poses is None:
            poses = self._poses(R, t, disp.shape[0])
        hip.tsdf_integrate(self.buffer, disp, occ, conf, left_u8, poses,
                           **_binding_kwargs(fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min, occ_min, filtered),
                           origin=self.origin, voxel_size=self.voxel_size, trunc=self.trunc, max_weight=self.max_weight, carve=carve)
        return self

    def extract(self, min_weight: int = 1, capacity: Optional[int] = None, want_gradients: bool = True) -> TsdfSurface:
        """The surface as a point cloud: one point per sign change of the tsdf between two neighbouring voxels that both have at least
        ``min_weight`` frames.  capacity None = Nx*Ny*Nz points (a crossing needs two voxels, three axes: the true bound is 3 per voxel, which
        no surface reaches).  Two launches, no synchronisation, capturable."""
        Nx, Ny, Nz = self.dims
        cap = Nx * Ny * Nz if capacity is None else int(capacity)
        if cap < 0:
            raise ValueError("TsdfVolume.extract: negative capacity")
        if self._workspace is None:
            self._workspace = torch.empty((hip.tsdf_workspace_bytes(Nx, Ny, Nz),), device=self.device, dtype=torch.uint8)
        records = torch.empty((cap, 4), device=self.device, dtype=torch.int32)
        gradients = torch.empty((cap, 3), device=self.device, dtype=torch.float32) if want_gradients else None
        count = torch.empty((1,), device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            hip.tsdf_extract(self.buffer, origin=self.origin, voxel_size=self.voxel_size, min_weight=min_weight, workspace=self._workspace,
                             records=records, gradients=gradients, count=count)
        return TsdfSurface(records[None], count, gradients)

    def extract_mesh(self, min_weight: int = 1, capacity: Optional[int] = None, face_capacity: Optional[int] = None,
                     want_gradients: bool = True) -> TsdfMesh:
        """The surface as a triangle mesh (K25, ``s2m2_tsdf_mesh``): ``extract``'s points as vertices, joined by marching cubes over the cells
        whose eight voxels all have at least ``min_weight`` frames.  capacity None = Nx*Ny*Nz vertices as for ``extract``; face_capacity None =
        2*Nx*Ny*Nz faces (the true bound is 5 per cell, which no surface reaches; ``face_count`` tells).  It keeps a workspace of its own (4
        bytes per voxel).  Three launches, no synchronisation, capturable."""
        Nx, Ny, Nz = self.dims
        cap = Nx * Ny * Nz if capacity is None else int(capacity)
        fcap = 2 * Nx * Ny * Nz if face_capacity is None else int(face_capacity)
        if cap < 0 or fcap < 0:
            raise ValueError("TsdfVolume.extract_mesh: negative capacity")
        if self._mesh_workspace is None:
            self._mesh_workspace = torch.empty((hip.tsdf_mesh_workspace_bytes(Nx, Ny, Nz),), device=self.device, dtype=torch.uint8)
        records = torch.empty((cap, 4), device=self.device, dtype=torch.int32)
        gradients = torch.empty((cap, 3), device=self.device, dtype=torch.float32) if want_gradients else None
        count = torch.empty((1,), device=self.device, dtype=torch.int32)
        faces = torch.empty((fcap, 3), device=self.device, dtype=torch.int32)
        face_count = torch.empty((1,), device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            hip.tsdf_mesh(self.buffer, origin=self.origin, voxel_size=self.voxel_size, min_weight=min_weight, workspace=self._mesh_workspace,
                          records=records, gradients=gradients, count=count, faces=faces, face_count=face_count)
        return TsdfMesh(records[None], count, gradients, faces, face_count)

    def far_corner(self, R, t) -> float:
        """the largest distance from the centre of a camera (``p_cam = R @ p_world + t``; (3,3) / (3,) or batched) to a corner of the grid, on
        the host in double: no surface of the volume lies deeper along any ray"""
        R = np.asarray(torch.as_tensor(R).detach().cpu(), dtype=np.float64).reshape(-1, 3, 3)
        t = np.asarray(torch.as_tensor(t).detach().cpu(), dtype=np.float64).reshape(-1, 3)
        n = max(len(R), len(t))
        centre = -np.einsum("bji,bj->bi", np.broadcast_to(R, (n, 3, 3)), np.broadcast_to(t, (n, 3)))        # -R^T t
        ext = (np.asarray(self.dims, dtype=np.float64) - 1.0) * self.voxel_size
        corners = np.asarray(self.origin)[None] + np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64) * ext[None]
        return float(np.linalg.norm(corners[None] - centre[:, None], axis=2).max())

    def raycast(self, camera: Camera, R=None, t=None, *, min_weight: int = 1, z_near: float = 0.0, z_far: Optional[float] = None,
                step: Optional[float] = None, want_gradients: bool = True, want_image: bool = True, want_count: bool = True) -> TsdfRender:
        """What the volume holds, seen from ``camera`` (K26, ``s2m2_tsdf_raycast``; the rule: include/s2m2_hip.h, K26): the camera's size and
        intrinsics, and the pose(s) ``R``, ``t`` in ``integrate``'s shapes and convention (world -> camera; default: ``camera.R``,
        ``camera.t``).  Every ray is sampled at ``z_near + k * step`` below ``z_far`` and ends at the first change of the interpolated tsdf from
        non-negative to negative between two samples whose eight voxels all have at least ``min_weight`` frames.  ``step`` None = trunc / 2;
        ``z_far`` None = the largest distance from a camera centre to a corner of the grid (computed on the host: reads R and t there).  A
        march of more than 65536 steps is refused.  One launch, no synchronisation, capturable."""
        R = camera.R if R is None else R
        t = camera.t if t is None else t
        Rt = torch.as_tensor(R)
        B = Rt.shape[0] if Rt.dim() == 3 else 1
        poses = self._poses(R, t, B, "raycast")
        step = self.trunc / 2.0 if step is None else float(step)
        z_far = self.far_corner(R, t) if z_far is None else float(z_far)
        Ht, Wt = camera.height, camera.width
        depth = torch.empty((B, 1, Ht, Wt), device=self.device, dtype=torch.float32)
        gradients = torch.empty((B, 3, Ht, Wt), device=self.device, dtype=torch.float32) if want_gradients else None
        image = torch.empty((B, 3, Ht, Wt), device=self.device, dtype=torch.uint8) if want_image else None
        count = torch.empty((B,), device=self.device, dtype=torch.int32) if want_count else None
        hip.tsdf_raycast(self.buffer, poses, Ht=Ht, Wt=Wt, fx=camera.fx, fy=camera.fy, cx=camera.cx, cy=camera.cy, origin=self.origin,
                         voxel_size=self.voxel_size, min_weight=min_weight, z_near=z_near, z_far=z_far, step=step, depth=depth,
                         gradients=gradients, image=image, count=count)
        return TsdfRender(depth, gradients, image, count, poses.view(B, 3, 4)[:, :, :3], poses, camera)

    def track(self, disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, render: TsdfRender, *, R=None, t=None, poses=None, fx: float,
              cx: float, cy: float, baseline: float, H: Optional[int] = None, W: Optional[int] = None, doffs: float = 0.0,
              fy: Optional[float] = None, depth_scale: float = 1000.0, depth_trunc: Optional[float] = None, conf_min: float = 0.1,
              occ_min: float = 0.5, filtered: bool = True, max_dist: Optional[float] = None, n_iters: int = 10, min_count: int = 100,
              max_rot: float = 0.2, max_trans: Optional[float] = None, want_systems: bool = True, want_residual: bool = False) -> TsdfTrack:
        """The pose of a new frame against the volume (K27, ``s2m2_tsdf_track``; the rule: include/s2m2_hip.h, K27): the live maps in
        ``reproject``'s conventions (``H``, ``W``: the fused crop, default the maps' own size) are registered by ``n_iters`` iterations of
        point-to-plane ICP with projective association to ``render``, a ``raycast`` of this volume WITH gradients from a nearby pose.  The
        initial guess is ``R``, ``t`` in ``integrate``'s shapes, or ``poses``: a device (B,12) fp32 buffer that is refined IN PLACE (the one
        ``integrate(poses=...)`` and the next ``raycast`` may read).  Defaults: ``max_dist`` = trunc (the correspondence gate), ``min_count``
        = 100 correspondences, ``max_rot`` = 0.2 rad and ``max_trans`` = 4 * trunc per iteration; an iteration that fails one of them leaves
        the pose as it was (``TsdfTrack.status``).  2 * n_iters launches, no synchronisation, capturable together with ``raycast`` and
        ``integrate``."""
        if render.gradients_buf is None or render.poses is None or render.camera is None:
            raise ValueError("TsdfVolume.track: the render must come from raycast(..., want_gradients=True)")
        B = disp.shape[0]
        if (poses is None) == (R is None or t is None):
            raise ValueError("TsdfVolume.track: pass the initial guess either as R and t or as poses")
        if poses is None:
            poses = self._poses(R, t, B, "track")
        Hl = disp.shape[2] if H is None else int(H)
        Wl = disp.shape[3] if W is None else int(W)
        need = hip.tsdf_track_workspace_bytes(B, Hl, Wl)
        if self._track_workspace is None or self._track_workspace.nbytes < need:
            self._track_workspace = torch.empty((need // 8,), device=self.device, dtype=torch.float64)
        n_iters = int(n_iters)
        systems = torch.empty((B, n_iters, 32), device=self.device, dtype=torch.float64) if want_systems else None
        residual = torch.empty((B, 1, Hl, Wl), device=self.device, dtype=torch.float32) if want_residual else None
        kw = _binding_kwargs(fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min, occ_min, filtered)
        cam = render.camera
        hip.tsdf_track(disp, occ, conf, poses, render.poses, render.depth, render.gradients_buf, H=Hl, W=Wl, **kw, mfx=cam.fx, mfy=cam.fy,
                       mcx=cam.cx, mcy=cam.cy, max_dist=self.trunc if max_dist is None else max_dist, min_count=min_count, max_rot=max_rot,
                       max_trans=4.0 * self.trunc if max_trans is None else max_trans, n_iters=n_iters, workspace=self._track_workspace,
                       systems=systems, residual=residual)
        return TsdfTrack(poses, systems, residual)


class NormalMap(TsdfRender):
    """What ``normals`` returns: a ``TsdfRender`` of the frame itself -- ``depth`` (B,1,H,W) fp32 K15's z (0: not kept), ``gradients_buf``
    (B,3,H,W) fp32 the UNIT normals in the camera frame, towards the camera (0,0,0: no normal), ``image`` (B,3,H,W) uint8 or None (the normal
    as a colour), ``count`` (B) int32 pixels with a normal or None, ``poses`` a device (B,12) identity and ``camera`` the frame's own.  So
    ``normals()`` and ``holes()`` work, and it stands wherever K27 takes a render: ``track(..., model=this)``."""


_TRACK_WORKSPACES: Dict[torch.device, torch.Tensor] = {}


def normals(disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, *, H: Optional[int] = None, W: Optional[int] = None, fx: float,
            cx: float, cy: float, baseline: float, doffs: float = 0.0, fy: Optional[float] = None, depth_scale: float = 1000.0,
            depth_trunc: Optional[float] = None, conf_min: float = 0.1, occ_min: float = 0.5, filtered: bool = True, radius: int = 1,
            max_jump: float = 1.0, min_cos: float = 0.0, want_image: bool = False, want_count: bool = True) -> NormalMap:
    """``reproject``'s maps and conventions (no image: ``H`` and ``W`` name the fused crop, default the maps' own size) -> NormalMap (K28,
    ``s2m2_normals``; the rule: include/s2m2_hip.h, K28).  The normal of a kept pixel is the cross product of the vertical and the horizontal
    difference of the points ``radius`` (1..8) pixels away -- central where both neighbours are kept and their disparities differ from the
    pixel's by at most ``max_jump * radius`` (``mesh``'s gate; inf joins every kept neighbour), one-sided where one is --, normalised, and kept
    where its cosine with the direction to the camera is at least ``min_cos``.  Only allocates: one launch, no synchronisation, capturable."""
    B, _, Hp, Wp = disp.shape
    H = Hp if H is None else int(H)
    W = Wp if W is None else int(W)
    dev = disp.device
    depth = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32)
    nrm = torch.empty((B, 3, H, W), device=dev, dtype=torch.float32)
    image = torch.empty((B, 3, H, W), device=dev, dtype=torch.uint8) if want_image else None
    count = torch.empty((B,), device=dev, dtype=torch.int32) if want_count else None
    kw = _binding_kwargs(fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min, occ_min, filtered)
    hip.normals(disp, occ, conf, H=H, W=W, **kw, radius=radius, max_jump=max_jump, min_cos=min_cos, depth=depth, normals=nrm, image=image,
                count=count)
    poses = torch.eye(3, 4, device=dev, dtype=torch.float32).reshape(1, 12).repeat(B, 1)
    return NormalMap(depth, nrm, image, count, poses.view(B, 3, 4)[:, :, :3], poses, Camera(W, H, kw["fx"], kw["fy"], cx, cy))


class Smoothed:
    """What ``smooth`` returns, all on the device: ``disp`` (B,1,Hp,Wp) fp32, the PADDED smoothed disparity with -1 wherever the pixel is not
    kept (border included: ``Segments.disp``'s convention); ``taps`` (B,1,H,W) int32 or None (neighbours in the pixel's sum, itself included;
    0: not kept); ``count`` (B) int32 kept pixels or None."""

    def __init__(self, disp: torch.Tensor, taps: Optional[torch.Tensor], count: Optional[torch.Tensor]):
        self.disp, self.taps, self.count = disp, taps, count

    def kept(self, b: int = 0) -> int:
        """kept pixels of pair b -- reads ``count`` on the host (synchronises)"""
        if self.count is None:
            raise ValueError("Smoothed.kept: smooth was called with want_count=False")
        return int(self.count[b].item())


def smooth(disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, *, H: Optional[int] = None, W: Optional[int] = None, fx: float,
           cx: float, cy: float, baseline: float, doffs: float = 0.0, fy: Optional[float] = None, depth_scale: float = 1000.0,
           depth_trunc: Optional[float] = None, conf_min: float = 0.1, occ_min: float = 0.5, filtered: bool = True, radius: int = 2,
           sigma_s: Optional[float] = None, sigma_r: float, max_jump: float, want_taps: bool = False, want_count: bool = True) -> Smoothed:
    """``reproject``'s maps and conventions (no image: ``H`` and ``W`` name the fused crop, default the maps' own size) -> Smoothed (K29,
    ``s2m2_smooth``; the rule: include/s2m2_hip.h, K29).  A bilateral filter: every kept pixel becomes the weighted mean of the kept pixels of
    its (2 ``radius`` + 1)^2 window (radius 1..8) whose disparities differ from its own by at most ``max_jump`` px -- NOT scaled by the radius
    --, weighted by a Gaussian of the distance (``sigma_s`` pixels, None: ``radius / 2``) times a Gaussian of the disparity difference
    (``sigma_r`` px).  ``sigma_r`` and ``max_jump`` have no default: they depend on the rig's disparity noise (a few sigma of it, and less
    than the smallest step that must stay an edge).  Only allocates: one launch, no synchronisation, capturable.

    Composition: ``s = smooth(...)`` then ``normals(s.disp, occ, conf, ..., filtered=False)`` (or ``reproject`` / ``mesh`` / ``register`` /
    ``voxelize`` / ``TsdfVolume.integrate`` / ``track``) sees exactly the kept pixels with their smoothed disparities -- whenever K15 itself
    drops d <= 0, that is whenever ``1e9 / depth_scale >= depth_trunc``.  With ``depth_trunc=None`` K15 keeps d <= 0 at z = 1e6 (depth_scale
    1000) as the reference's formula does, the dropped pixels included: pass a real truncation distance to the stage behind.  After
    ``segment``, pass ``segment(...).disp`` in with ``filtered=False``, so that speckles are removed before they are averaged into their
    surroundings."""
    B, _, Hp, Wp = disp.shape
    H = Hp if H is None else int(H)
    W = Wp if W is None else int(W)
    dev = disp.device
    out = torch.empty((B, 1, Hp, Wp), device=dev, dtype=torch.float32)
    taps = torch.empty((B, 1, H, W), device=dev, dtype=torch.int32) if want_taps else None
    count = torch.empty((B,), device=dev, dtype=torch.int32) if want_count else None
    kw = _binding_kwargs(fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min, occ_min, filtered)
    hip.smooth(disp, occ, conf, H=H, W=W, **kw, radius=radius, sigma_s=radius / 2.0 if sigma_s is None else sigma_s, sigma_r=sigma_r,
               max_jump=max_jump, disp_out=out, taps=taps, count=count)
    return Smoothed(out, taps, count)


def track(disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, model: TsdfRender, *, R=None, t=None, poses: Optional[torch.Tensor] = None,
          fx: float, cx: float, cy: float, baseline: float, doffs: float = 0.0, fy: Optional[float] = None, depth_scale: float = 1000.0,
          depth_trunc: Optional[float] = None, conf_min: float = 0.1, occ_min: float = 0.5, filtered: bool = True, H: Optional[int] = None,
          W: Optional[int] = None, max_dist: float, max_trans: float, n_iters: int = 10, min_count: int = 100, max_rot: float = 0.2,
          want_systems: bool = True, want_residual: bool = False) -> TsdfTrack:
    """K27 (``s2m2_tsdf_track``) without a volume: the live maps in ``reproject``'s conventions (``H``, ``W``: the fused crop, default the maps'
    own size) are registered to ``model``, any ``TsdfRender`` with gradients, poses and a camera -- a ``NormalMap`` of the previous frame
    makes this frame-to-frame odometry: the result is the pose of the live camera in the previous frame's.  The initial guess is ``R``, ``t``
    in ``TsdfVolume.integrate``'s shapes, or ``poses``: a device (B,12) fp32 buffer that is refined IN PLACE; with none of them the identity.
    ``max_dist`` (the correspondence gate) and ``max_trans`` (the longest step of an iteration), both in the unit of z, have no default: there
    is no truncation distance to derive them from.  The workspace is kept per device from the first call on (make that call outside a
    capture).  2 * n_iters launches, no synchronisation, capturable together with ``normals``."""
    if model.gradients_buf is None or model.poses is None or model.camera is None:
        raise ValueError("track: the model must carry gradients, poses and a camera (normals(...), or raycast(..., want_gradients=True))")
    B = disp.shape[0]
    dev = disp.device
    if poses is not None and (R is not None or t is not None):
        raise ValueError("track: pass the initial guess either as R and t or as poses")
    if poses is None:
        if (R is None) != (t is None):
            raise ValueError("track: R and t come together")
        if R is None:
            poses = torch.eye(3, 4, device=dev, dtype=torch.float32).reshape(1, 12).repeat(B, 1)
        else:
            R = torch.as_tensor(R).to(device=dev, dtype=torch.float32)
            t = torch.as_tensor(t).to(device=dev, dtype=torch.float32)
            if tuple(R.shape) not in ((3, 3), (B, 3, 3)) or tuple(t.shape) not in ((3,), (B, 3)):
                raise ValueError(f"track: R is (3,3) or ({B},3,3) and t is (3,) or ({B},3), got {tuple(R.shape)} and {tuple(t.shape)}")
            poses = torch.cat([R.expand(B, 3, 3), t.expand(B, 3)[:, :, None]], dim=2).reshape(B, 12).contiguous()
    Hl = disp.shape[2] if H is None else int(H)
    Wl = disp.shape[3] if W is None else int(W)
    need = hip.tsdf_track_workspace_bytes(B, Hl, Wl)
    workspace = _TRACK_WORKSPACES.get(dev)
    if workspace is None or workspace.nbytes < need:
        workspace = _TRACK_WORKSPACES[dev] = torch.empty((need // 8,), device=dev, dtype=torch.float64)
    n_iters = int(n_iters)
    systems = torch.empty((B, n_iters, 32), device=dev, dtype=torch.float64) if want_systems else None
    residual = torch.empty((B, 1, Hl, Wl), device=dev, dtype=torch.float32) if want_residual else None
    kw = _binding_kwargs(fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min, occ_min, filtered)
    cam = model.camera
    hip.tsdf_track(disp, occ, conf, poses, model.poses, model.depth, model.gradients_buf, H=Hl, W=Wl, **kw, mfx=cam.fx, mfy=cam.fy, mcx=cam.cx,
                   mcy=cam.cy, max_dist=max_dist, min_count=min_count, max_rot=max_rot, max_trans=max_trans, n_iters=n_iters,
                   workspace=workspace, systems=systems, residual=residual)
    return TsdfTrack(poses, systems, residual)
