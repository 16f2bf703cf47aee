"""numpy oracle of K24 (include/s2m2_hip.h: s2m2_tsdf_integrate, s2m2_tsdf_extract), independent of the code under test.

The formulas of the header restated with float32 ARRAY arithmetic -- every elementwise numpy operation on float32 arrays is one IEEE
rounding, and nothing is fused --, vectorised over the voxels; keep, z and the colour bytes of a pixel come from cloud_oracle (K15's).
A volume is an (Nz, Ny, Nx, 4) int32 array: word 0 the tsdf's bits, word 1 the weight, word 2 r | g << 16, word 3 b | pad << 16.
"""
import numpy as np

import cloud_oracle

F = np.float32

# what happened to a voxel under one pair (integrate's `cls`): the skip classes of the header in their order, then UPDATED
BEHIND, OUTSIDE, NOT_KEPT, BELOW_BAND, IN_FRONT, UPDATED = range(6)


def empty(dims):
    Nx, Ny, Nz = dims
    return np.zeros((Nz, Ny, Nx, 4), np.int32)


def centres(dims, origin, voxel_size):
    """x, y, z (n) float32 of every voxel in lin order, and i, j, k"""
    Nx, Ny, Nz = dims
    k, j, i = (a.ravel() for a in np.meshgrid(np.arange(Nz), np.arange(Ny), np.arange(Nx), indexing="ij"))
    vs = F(voxel_size)
    return (F(origin[0]) + i.astype(F) * vs, F(origin[1]) + j.astype(F) * vs, F(origin[2]) + k.astype(F) * vs), (i, j, k)


def unpack(vol):
    v = vol.reshape(-1, 4).view(np.uint32)
    return dict(tsdf=v[:, 0].view(F).copy(), weight=v[:, 1].view(np.int32).copy(), r=v[:, 2] & 0xffff, g=v[:, 2] >> 16, b=v[:, 3] & 0xffff,
                pad=v[:, 3] >> 16)


def integrate(vol, disp, occ, conf, image, poses, *, origin, voxel_size, trunc, max_weight, carve=False, fx, fy, cx, cy, **cam):
    """vol (Nz,Ny,Nx,4) int32; disp / occ / conf (B,Hp,Wp) float32 PADDED; image (B,3,H,W); poses (B,12).  cam: the remaining keywords of
    cloud_oracle.cloud.  Returns (new volume, diag) with diag a list of one dict per pair: cls (n) the class of every voxel, up, vp, fu, fv, sdf, Z (n)
    and pix (n) the flat index of the pixel a voxel projects to (0 where it projects outside)."""
    B, _, H, W = image.shape
    Nz, Ny, Nx, _ = vol.shape
    out = vol.copy()
    v = out.reshape(-1, 4).view(np.uint32)
    tsdf, weight = v[:, 0].view(F).copy(), v[:, 1].view(np.int32).astype(np.int64)
    col = [(v[:, 2] & 0xffff).astype(np.uint64), (v[:, 2] >> 16).astype(np.uint64), (v[:, 3] & 0xffff).astype(np.uint64)]
    pad = v[:, 3] >> 16
    touched = np.zeros(len(v), bool)
    (x, y, z), _ = centres((Nx, Ny, Nz), origin, voxel_size)
    tr = F(trunc)
    diag = []
    for b in range(B):
        c = cloud_oracle.cloud(cloud_oracle.crop(disp[b], H, W), cloud_oracle.crop(occ[b], H, W), cloud_oracle.crop(conf[b], H, W), image[b],
                               fx=fx, fy=fy, cx=cx, cy=cy, **cam)
        rgb = cloud_oracle.colour_bytes(image[b]).reshape(3, H * W)
        q = np.asarray(poses[b], dtype=F)
        with np.errstate(all="ignore"):
            X = ((q[0] * x + q[1] * y) + q[2] * z) + q[3]
            Y = ((q[4] * x + q[5] * y) + q[6] * z) + q[7]
            Z = ((q[8] * x + q[9] * y) + q[10] * z) + q[11]
            front = (Z > 0) & np.isfinite(Z)
            up = (F(fx) * X) / Z + F(cx)
            vp = (F(fy) * Y) / Z + F(cy)
            fu, fv = np.rint(up), np.rint(vp)
            inside = front & (fu >= 0) & (fu < F(W)) & (fv >= 0) & (fv < F(H))
            pix = np.where(inside, fv, 0).astype(np.int64) * W + np.where(inside, fu, 0).astype(np.int64)
            kept = inside & c["keep"].ravel()[pix]
            sdf = c["depth"].ravel()[pix] - Z
            band = kept & (sdf >= -tr)
            upd = band & (bool(carve) | ~(sdf > tr))
            d = np.minimum(sdf / tr, F(1.0))
        cls = np.full(len(v), BEHIND, np.int8)
        cls[front] = OUTSIDE
        cls[inside] = NOT_KEPT
        cls[kept] = BELOW_BAND
        cls[band] = IN_FRONT
        cls[upd] = UPDATED
        diag.append(dict(cls=cls, up=up, vp=vp, fu=fu, fv=fv, pix=pix, sdf=sdf, Z=Z))
        n = np.flatnonzero(upd)
        Wf = weight[n].astype(F)
        tsdf[n] = (tsdf[n] * Wf + d[n]) / (Wf + F(1.0))
        w = weight[n].astype(np.uint64)
        for ch in range(3):
            num = col[ch][n] * w + (rgb[ch, pix[n]].astype(np.uint64) << np.uint64(8)) + ((w + np.uint64(1)) >> np.uint64(1))
            assert (num < 1 << 32).all()
            col[ch][n] = num // (w + np.uint64(1))
        weight[n] = np.minimum(weight[n] + 1, max_weight)
        touched[n] = True
    n = np.flatnonzero(touched)
    v[n, 0] = tsdf[n].view(np.uint32)
    v[n, 1] = weight[n].astype(np.uint32)
    v[n, 2] = ((col[0][n] & np.uint64(0xffff)) | (col[1][n] << np.uint64(16))).astype(np.uint32)
    v[n, 3] = ((col[2][n] & np.uint64(0xffff)).astype(np.uint32)) | (pad[n] << 16)
    return out, diag


def extract(vol, *, origin, voxel_size, min_weight=1):
    """-> dict: records (m,4) int32, gradients (m,3) float32, count m, lin (m) and axis (m) of every point's v0, far (m) bool: sel = v1"""
    Nz, Ny, Nx, _ = vol.shape
    dims = (Nx, Ny, Nz)
    u = unpack(vol)
    t, obs = u["tsdf"], u["weight"] >= min_weight
    (x, y, z), (i, j, k) = centres(dims, origin, voxel_size)
    pos = (i, j, k)
    stride = (1, Nx, Nx * Ny)
    n = len(t)
    lin = np.arange(n)

    def shifted(b, d):
        """index of the neighbour at distance d along axis b, and whether it is inside the grid"""
        ok = (pos[b] + d >= 0) & (pos[b] + d < dims[b])
        return np.where(ok, lin + d * stride[b], lin), ok

    emit = np.zeros((n, 3), bool)
    for a in range(3):
        nb, ok = shifted(a, 1)
        emit[:, a] = obs & ok & obs[nb] & ((t < 0) != (t[nb] < 0))
    flat = np.flatnonzero(emit.ravel())
    l0, ax = flat // 3, flat % 3
    l1 = l0 + np.take(stride, ax)
    t0, t1 = t[l0], t[l1]
    vs = F(voxel_size)
    with np.errstate(all="ignore"):
        s = t0 / (t0 - t1)
        xyz = np.stack([x[l0], y[l0], z[l0]], 1)
        m = np.arange(len(l0))
        xyz[m, ax] = xyz[m, ax] + s * vs
    far = np.abs(t1) < np.abs(t0)
    sel = np.where(far, l1, l0)
    rec = np.zeros((len(l0), 4), np.uint32)
    rec[:, :3] = xyz.astype(F).view(np.uint32)
    byte = [((u[c][sel].astype(np.uint32) + 128) >> 8) for c in "rgb"]
    rec[:, 3] = byte[0] | (byte[1] << 8) | (byte[2] << 16) | np.uint32(0xff000000)
    grad = np.zeros((len(l0), 3), F)
    for b in range(3):
        nbp, okp = shifted(b, 1)
        nbm, okm = shifted(b, -1)
        tp = np.where(okp & obs[nbp], t[nbp], t)
        tm = np.where(okm & obs[nbm], t[nbm], t)
        with np.errstate(all="ignore"):
            grad[:, b] = tp[sel] - tm[sel]
    return dict(records=rec.view(np.int32), gradients=grad, count=len(l0), lin=l0, axis=ax, far=far, observed=obs)
