"""numpy oracle of K23 (include/s2m2_hip.h: s2m2_voxel), independent of the code under test and written from the header line by line: the
points are ``cloud_oracle.cloud``'s (K15's keep, z, x32, y32 and colour bytes), the quantisation is one float32 division and ``np.rint`` in
float32, everything behind it is integer arithmetic (int64 sums with ``np.add.at``), the centroid is formed in float64 in the stated order,
and the records are ordered by the smallest raster index of their points."""
import numpy as np

import cloud_oracle

F = np.float32
RANGE = F(2.0 ** 30)


def quantise(x, q):
    """float32 array -> (X as float32 = rint(x / q), in range)"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        X = np.rint(np.asarray(x, dtype=F) / F(q)).astype(F)
        return X, np.abs(X) < RANGE


def key_of(ix, iy, iz):
    ix, iy, iz = (np.asarray(a, dtype=np.int64) for a in (ix, iy, iz))
    return ((ix + (1 << 20)) << 42) | ((iy + (1 << 20)) << 21) | (iz + (1 << 20))


def slots_of(max_voxels):
    """the smallest power of two >= 2 * max_voxels"""
    s = 2
    while s < 2 * max_voxels:
        s *= 2
    return s


def voxelize(disp, occ, conf, image, *, voxel_size, fx, fy, cx, cy, baseline, doffs=0.0, depth_scale=1000.0, depth_trunc=None, conf_min=0.1,
             occ_min=0.5, filtered=True):
    """One pair, maps ALREADY cropped (H,W), image (3,H,W).  Returns a dict: records (n,4) int32 (the 16-byte records as words), weights (n)
    int32, index (H,W) int32, stats [kept, out of range, 0, n], voxels (n,3) int64 = (ix, iy, iz) of every record, first (n) int64."""
    c = cloud_oracle.cloud(disp, occ, conf, image, fx=fx, fy=fy, cx=cx, cy=cy, baseline=baseline, doffs=doffs, depth_scale=depth_scale,
                           depth_trunc=depth_trunc, conf_min=conf_min, occ_min=occ_min, filtered=filtered)
    H, W = c["keep"].shape
    q = F(voxel_size) / F(1024.0)
    X, okx = quantise(c["x32"], q)
    Y, oky = quantise(c["y32"], q)
    Z, okz = quantise(c["z"], q)
    ok = okx & oky & okz
    pix = c["index"][ok]                                      # raster indices of the points that count, ascending
    Xi, Yi, Zi = (a[ok].astype(np.int64) for a in (X, Y, Z))
    ix, iy, iz = Xi >> 10, Yi >> 10, Zi >> 10                # floor
    local = np.stack([Xi & 1023, Yi & 1023, Zi & 1023], axis=1)
    keys, first_pos, inverse = np.unique(key_of(ix, iy, iz), return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    nv = len(keys)
    n = np.zeros(nv, np.int64)
    np.add.at(n, inverse, 1)
    sums = np.zeros((nv, 3), np.int64)
    np.add.at(sums, inverse, local)
    csum = np.zeros((nv, 3), np.int64)
    np.add.at(csum, inverse, c["rgb"][ok].astype(np.int64))
    first = np.full(nv, np.iinfo(np.int64).max)
    np.minimum.at(first, inverse, pix)
    order = np.argsort(first, kind="stable")
    rank_of = np.empty(nv, np.int64)
    rank_of[order] = np.arange(nv)
    cell = np.stack([ix, iy, iz], axis=1)[first_pos]          # (nv,3): the voxel of every key
    centre = ((cell.astype(np.float64) * 1024.0 + sums.astype(np.float64) / n.astype(np.float64)[:, None]) * np.float64(q)).astype(F)
    colour = ((2 * csum + n[:, None]) // (2 * n[:, None])).astype(np.uint8)
    rec = np.zeros((nv, 4), np.int32)
    rec[:, :3] = centre.view(np.int32)
    rgba = np.concatenate([colour, np.full((nv, 1), 255, np.uint8)], axis=1)
    rec[:, 3] = np.ascontiguousarray(rgba).view("<u4").reshape(-1).view(np.int32)
    index = np.full(H * W, -1, np.int32)
    index[pix] = rank_of[inverse]
    return dict(records=rec[order], weights=n[order].astype(np.int32), index=index.reshape(H, W),
                stats=np.array([len(c["index"]), int((~ok).sum()), 0, nv], np.int32), voxels=cell[order], first=first[order], keep=c["keep"])
