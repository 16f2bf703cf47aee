"""numpy oracle of K25 (include/s2m2_hip.h: s2m2_tsdf_mesh), independent of the code under test.

The vertices are tsdf_oracle.extract's points (that is K25's definition); the emit flags and the ranks are computed here a second time, and the
faces come from the case table of s2m2_amd/mc_table.py: build_table(), the generator the kernel's header is written by.  A volume is an
(Nz, Ny, Nx, 4) int32 array as in tsdf_oracle.
"""
import numpy as np

import tsdf_oracle
from s2m2_amd import mc_table

TABLE = mc_table.build_table()
MAX_TRIANGLES = mc_table.max_triangles(TABLE)
COUNTS = np.array([len(t) for t in TABLE], np.int64)
TRIS = np.zeros((256, MAX_TRIANGLES, 3), np.int64)                     # case, triangle, corner -> edge number
for _case, _tris in enumerate(TABLE):
    for _t, _tri in enumerate(_tris):
        TRIS[_case, _t] = _tri
EDGE_AXIS = np.array([a for a, _ in mc_table.EDGES], np.int64)
EDGE_BASE = np.array([b for _, b in mc_table.EDGES], np.int64)


def cells(vol, min_weight=1):
    """-> (case, valid), both (Nz-1, Ny-1, Nx-1): the case of every cell and whether all eight of its corners are observed"""
    Nz, Ny, Nx, _ = vol.shape
    u = tsdf_oracle.unpack(vol)
    neg = (u["tsdf"] < 0).reshape(Nz, Ny, Nx)
    obs = (u["weight"] >= min_weight).reshape(Nz, Ny, Nx)
    case = np.zeros((max(Nz - 1, 0), max(Ny - 1, 0), max(Nx - 1, 0)), np.int64)
    valid = np.ones(case.shape, bool)
    for c in range(8):
        dx, dy, dz = c & 1, c >> 1 & 1, c >> 2
        sl = (slice(dz, Nz - 1 + dz), slice(dy, Ny - 1 + dy), slice(dx, Nx - 1 + dx))
        case |= neg[sl].astype(np.int64) << c
        valid &= obs[sl]
    return case, valid


def mesh(vol, *, origin, voxel_size, min_weight=1):
    """-> tsdf_oracle.extract's dict plus faces (m,3) int32 of vertex ranks, face_count m, face_cell (m) the lin of every face's cell, and
    case / valid of cells()"""
    Nz, Ny, Nx, _ = vol.shape
    n = Nx * Ny * Nz
    e = tsdf_oracle.extract(vol, origin=origin, voxel_size=voxel_size, min_weight=min_weight)
    # the emit flags and the ranks once more, from the definition
    u = tsdf_oracle.unpack(vol)
    t = u["tsdf"].reshape(Nz, Ny, Nx)
    obs = (u["weight"] >= min_weight).reshape(Nz, Ny, Nx)
    emit = np.zeros((Nz, Ny, Nx, 3), bool)
    emit[:, :, :-1, 0] = obs[:, :, :-1] & obs[:, :, 1:] & ((t[:, :, :-1] < 0) != (t[:, :, 1:] < 0))
    emit[:, :-1, :, 1] = obs[:, :-1] & obs[:, 1:] & ((t[:, :-1] < 0) != (t[:, 1:] < 0))
    emit[:-1, :, :, 2] = obs[:-1] & obs[1:] & ((t[:-1] < 0) != (t[1:] < 0))
    flat = emit.reshape(-1)
    rank = (np.cumsum(flat) - flat).reshape(n, 3)                       # (voxel, axis) -> rank of its point, where it emits one
    assert int(flat.sum()) == e["count"]

    case, valid = cells(vol, min_weight)
    kk, jj, ii = np.nonzero(valid & (COUNTS[case] > 0))                 # ascending lin
    cs = case[kk, jj, ii]
    lin = (kk * Ny + jj) * Nx + ii
    per = COUNTS[cs]
    which = np.repeat(np.arange(len(cs)), per)                          # face -> its cell
    tri = np.arange(int(per.sum())) - np.repeat(np.cumsum(per) - per, per)
    edges = TRIS[cs[which], tri]                                        # (m,3) edge numbers
    a, b = EDGE_AXIS[edges], EDGE_BASE[edges]
    voxel = lin[which][:, None] + (b & 1) + (b >> 1 & 1) * Nx + (b >> 2) * Nx * Ny
    assert emit.reshape(n, 3)[voxel, a].all()                           # in a valid cell every sign-changing edge has its point
    faces = rank[voxel, a].astype(np.int32)
    out = dict(e)
    out.update(faces=faces.reshape(-1, 3), face_count=len(faces), face_cell=lin[which], case=case, valid=valid)
    return out
