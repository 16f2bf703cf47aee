"""numpy oracle of K28 (include/s2m2_hip.h: s2m2_normals), independent of the code under test.

The per-pixel rule of the header restated with float32 ARRAY arithmetic -- every elementwise numpy operation on float32 arrays is one IEEE
rounding, and nothing is fused --, vectorised over the pixels of one pair; keep and z of a pixel come from cloud_oracle (K15's), on the
CROPPED maps, so a padded pixel can never be a neighbour.  np.sqrt and the division of float32 arrays are correctly rounded, as the rule
requires of the kernel.  ``normals`` takes the switches of the wrong kernels of test_normals_cpu.py; all of them default to the rule.
"""
import numpy as np

import cloud_oracle

F = np.float32

# what happened to a pixel: the hole reasons of the header in their order, then USED
NOT_KEPT, NO_HORIZONTAL, NO_VERTICAL, DEGENERATE, GRAZING, USED = range(6)
CLASS_NAMES = ("not kept", "no horizontal neighbour", "no vertical neighbour", "degenerate", "grazing", "used")


def _shift(a, dv, du, fill):
    """out[v, u] = a[v + dv, u + du] where that lies inside the array, else fill"""
    H, W = a.shape
    out = np.full_like(a, fill)
    v0, v1, u0, u1 = max(0, -dv), min(H, H - dv), max(0, -du), min(W, W - du)
    if v0 < v1 and u0 < u1:
        out[v0:v1, u0:u1] = a[v0 + dv:v1 + dv, u0 + du:u1 + du]
    return out


def normals(disp, occ, conf, *, H, W, fx, fy, cx, cy, radius=1, max_jump=1.0, min_cos=0.0, central_only=False, gate_far=False,
            gate_unscaled=False, swapped=False, no_crop=False, radius_one=False, padded_neighbours=False, view_z=False, **cam):
    """One pair.  disp / occ / conf (Hp,Wp) float32 PADDED; cam: the remaining keywords of cloud_oracle.cloud (baseline, doffs, depth_scale,
    depth_trunc, conf_min, occ_min, filtered).  -> dict: depth (H,W) float32, normals (3,H,W) float32, image (3,H,W) uint8, count, cls (H,W)
    int8.  The keywords behind min_cos are the WRONG kernels of the CPU test."""
    Hp, Wp = disp.shape
    oy, ox = (0, 0) if no_crop else ((Hp - H) // 2, (Wp - W) // 2)
    r = 1 if radius_one else int(radius)
    if padded_neighbours:                                    # evaluate the whole padded map and crop the RESULT: the border becomes a neighbour
        full = normals(disp, occ, conf, H=Hp, W=Wp, fx=fx, fy=fy, cx=float(F(cx) + F(ox)), cy=float(F(cy) + F(oy)), radius=radius,
                       max_jump=max_jump, min_cos=min_cos, **cam)
        out = {k: np.ascontiguousarray(full[k][..., oy:oy + H, ox:ox + W]) for k in ("depth", "normals", "image", "cls")}
        out["count"] = int((out["cls"] == USED).sum())
        return out
    win = lambda m: np.ascontiguousarray(np.asarray(m, F)[oy:oy + H, ox:ox + W])
    d = win(disp)
    c = cloud_oracle.cloud(d, win(occ), win(conf), np.zeros((3, H, W), np.uint8), fx=fx, fy=fy, cx=cx, cy=cy, **cam)
    keep, z = c["keep"], c["depth"].astype(F)
    v, u = np.mgrid[0:H, 0:W]
    gate = F(max_jump) if gate_unscaled else F(max_jump) * F(radius)
    with np.errstate(all="ignore"):
        x = (u.astype(F) - F(cx)) * z / F(fx)
        y = (v.astype(F) - F(cy)) * z / F(fy)
        P = (x, y, z)

        def pair(dv, du):
            """the difference of one pair of neighbours, plus = (v + dv, u + du), minus = (v - dv, u - du) -> (3 arrays, has)"""
            side = []
            for s in (1, -1):
                kq, dq = _shift(keep, s * dv, s * du, False), _shift(d, s * dv, s * du, F(0))
                Pq = [_shift(a, s * dv, s * du, F(0)) for a in P]
                side.append((kq, dq, Pq))
            (kp, dp, Pp), (km, dm, Pm) = side
            if gate_far:                                     # WRONG: the jump measured between the two neighbours
                up = kp & (np.abs(dp - dm) <= gate)
                um = km & (np.abs(dm - dp) <= gate)
            else:
                up = kp & (np.abs(dp - d) <= gate)
                um = km & (np.abs(dm - d) <= gate)
            if central_only:                                 # WRONG: no one-sided differences
                up = um = up & um
            a = [np.where(up, Pp[i], P[i]) for i in range(3)]
            b = [np.where(um, Pm[i], P[i]) for i in range(3)]
            return [a[i] - b[i] for i in range(3)], up | um

        dx, hx = pair(0, r)
        dy, hy = pair(r, 0)
        if swapped:                                          # WRONG: dx x dy
            dx, dy = dy, dx
        nx = dy[1] * dx[2] - dy[2] * dx[1]
        ny = dy[2] * dx[0] - dy[0] * dx[2]
        nz = dy[0] * dx[1] - dy[1] * dx[0]
        s = (nx * nx + ny * ny) + nz * nz
        good = (s > 0) & np.isfinite(s)
        q = np.sqrt(s)
        n = [nx / q, ny / q, nz / q]
        if view_z:                                           # WRONG: the view gate on z alone
            cosv = -n[2]
        else:
            m = np.sqrt((x * x + y * y) + z * z)
            cosv = -(((n[0] * x + n[1] * y) + n[2] * z) / m)
        facing = cosv >= F(min_cos)
    assert all(a.dtype == F for a in n) and cosv.dtype == F and s.dtype == F
    cls = np.full((H, W), NOT_KEPT, np.int8)
    cls[keep] = NO_HORIZONTAL
    cls[keep & hx] = NO_VERTICAL
    cls[keep & hx & hy] = DEGENERATE
    cls[keep & hx & hy & good] = GRAZING
    used = keep & hx & hy & good & facing
    cls[used] = USED
    nrm = np.stack([np.where(used, a, F(0)) for a in n]).astype(F)
    with np.errstate(all="ignore"):
        byte = np.rint(nrm * F(127.5) + F(127.5))
    image = np.where(used[None], byte, F(0)).astype(np.uint8)
    return dict(depth=c["depth"].astype(F), normals=nrm, image=image, count=int(used.sum()), cls=cls)


def batch(disp, occ, conf, **kw):
    """disp / occ / conf (B,Hp,Wp) -> dict: depth (B,1,H,W), normals (B,3,H,W), image (B,3,H,W), count (B) int32, cls (B,H,W)"""
    outs = [normals(disp[b], occ[b], conf[b], **kw) for b in range(len(disp))]
    return dict(depth=np.stack([o["depth"] for o in outs])[:, None], normals=np.stack([o["normals"] for o in outs]),
                image=np.stack([o["image"] for o in outs]), count=np.array([o["count"] for o in outs], np.int32),
                cls=np.stack([o["cls"] for o in outs]))
