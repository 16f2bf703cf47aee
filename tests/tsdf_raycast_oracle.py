"""numpy oracle of K26 (include/s2m2_hip.h: s2m2_tsdf_raycast), independent of the code under test.

The rule of the header restated with float32 ARRAY arithmetic -- every elementwise numpy operation on float32 arrays is one IEEE rounding, and
nothing is fused --, vectorised over the pixels of one pair, with a Python loop over the samples k.  No sample is skipped: what the kernel may
leave out is decided here by the rule alone.  A volume is tsdf_oracle's (Nz, Ny, Nx, 4) int32 array.
"""
import math

import numpy as np

F = np.float32
MAX_STEPS = 65536


def n_steps(z_near, z_far, step):
    """ceil((z_far - z_near) / step) in double from the float32 values"""
    return int(math.ceil((float(F(z_far)) - float(F(z_near))) / float(F(step))))


def _rays(q, Ht, Wt, fx, fy, cx, cy, origin, voxel_size):
    """a, b (3, Ht*Wt) float32 of every pixel in raster order: the position in voxel units at depth z is a + z * b"""
    v, u = (x.ravel() for x in np.mgrid[0:Ht, 0:Wt])
    q = np.asarray(q, dtype=F)
    vs = F(voxel_size)
    with np.errstate(all="ignore"):
        dx = (u.astype(F) - F(cx)) / F(fx)
        dy = (v.astype(F) - F(cy)) / F(fy)
        a, b = [], []
        for c in range(3):                                   # column c of R: q[c], q[4 + c], q[8 + c]
            w = (q[c] * dx + q[4 + c] * dy) + q[8 + c]
            o = -((q[c] * q[3] + q[4 + c] * q[7]) + q[8 + c] * q[11])
            a.append(np.full(len(u), (o - F(origin[c])) / vs, F))
            b.append(w / vs)
    return np.stack(a), np.stack(b)


def _lerp(lo, hi, fr):
    return lo + fr * (hi - lo)


def _sample(tsdf, obs, dims, a, b, z):
    """the samples at depth z (array or scalar) of the rays a, b -> observed (n) bool, t (n), corners (8, n), fr (3, n), lin (n) of corner 0"""
    Nx, Ny, Nz = dims
    with np.errstate(all="ignore"):
        g = a + z * b
        f0 = np.floor(g)
        inside = np.ones(g.shape[1], bool)
        for c, N in enumerate(dims):
            inside &= (f0[c] >= 0) & (f0[c] <= F(N - 2))             # a NaN or Inf fails
        i0 = np.where(inside, f0, 0).astype(np.int64)
        lin = (i0[2] * Ny + i0[1]) * Nx + i0[0]
        off = [(c & 1) + ((c >> 1) & 1) * Nx + (c >> 2) * Nx * Ny for c in range(8)]
        ok = inside.copy()
        corners = np.zeros((8, g.shape[1]), F)
        for c in range(8):
            idx = np.where(inside, lin + off[c], 0)
            ok &= obs[idx]
            corners[c] = tsdf[idx]
        fr = (g - f0).astype(F)
        c00, c10 = _lerp(corners[0], corners[1], fr[0]), _lerp(corners[2], corners[3], fr[0])
        c01, c11 = _lerp(corners[4], corners[5], fr[0]), _lerp(corners[6], corners[7], fr[0])
        t = _lerp(_lerp(c00, c10, fr[1]), _lerp(c01, c11, fr[1]), fr[2])
    return ok, t, corners, fr, lin


def raycast(vol, poses, *, Ht, Wt, fx, fy, cx, cy, origin, voxel_size, min_weight=1, z_near=0.0, z_far, step):
    """vol (Nz,Ny,Nx,4) int32; poses (B,12) -> dict: depth (B,1,Ht,Wt) float32, gradients (B,3,Ht,Wt) float32, image (B,3,Ht,Wt) uint8, count
    (B) int32, and the diagnostics, each (B,Ht,Wt): steps (the k of the crossing, -1: none), reset (have_prev went from true to false before
    the crossing), hit_unobserved (a crossing whose hit sample is unobserved: a hole), fr_hit (B,3,Ht,Wt) of the covered pixels (else NaN),
    t_prev (B,Ht,Wt) the value in front of the crossing (NaN: none), on_centre (the march met an observed sample with fr == 0 on all axes),
    on_edge (the march met a sample with g == N - 1 exactly on an axis and inside the grid on the others: unobserved by its position alone)"""
    Nz, Ny, Nx, _ = vol.shape
    dims = (Nx, Ny, Nz)
    words = vol.reshape(-1, 4).view(np.uint32)
    tsdf = words[:, 0].view(F)
    obs = words[:, 1].view(np.int32) >= min_weight
    col = np.stack([words[:, 2] & 0xffff, words[:, 2] >> 16, words[:, 3] & 0xffff])
    B, n = len(poses), Ht * Wt
    K = n_steps(z_near, z_far, step)
    assert 1 <= K <= MAX_STEPS
    zn, st = F(z_near), F(step)
    out = dict(depth=np.zeros((B, 1, Ht, Wt), F), gradients=np.zeros((B, 3, Ht, Wt), F), image=np.zeros((B, 3, Ht, Wt), np.uint8),
               count=np.zeros(B, np.int32), steps=np.full((B, Ht, Wt), -1, np.int32), reset=np.zeros((B, Ht, Wt), bool),
               hit_unobserved=np.zeros((B, Ht, Wt), bool), fr_hit=np.full((B, 3, Ht, Wt), np.nan, F), n_steps=K,
               t_prev=np.full((B, Ht, Wt), np.nan, F), on_centre=np.zeros((B, Ht, Wt), bool), on_edge=np.zeros((B, Ht, Wt), bool))
    for bi in range(B):
        a, b = _rays(poses[bi], Ht, Wt, fx, fy, cx, cy, origin, voxel_size)
        have_prev, done, reset = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
        t_prev, z_prev, t_hit, z_at = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
        steps = np.full(n, -1, np.int32)
        on_centre, on_edge = np.zeros(n, bool), np.zeros(n, bool)
        for k in range(K):
            live = ~done
            if not live.any():
                break
            z_k = zn + F(k) * st
            ok, t, _, fr, _ = _sample(tsdf, obs, dims, a, b, z_k)
            with np.errstate(all="ignore"):
                g = a + z_k * b
                top = np.array(dims, F)[:, None] - F(1)
                on_edge |= live & ((g == top).any(0)) & ((g >= 0) & (g <= top)).all(0)
            on_centre |= live & ok & (fr == 0).all(0)
            lost = live & ~ok
            reset |= lost & have_prev
            have_prev[lost] = False
            cross = live & ok & have_prev & ~(t_prev < 0) & (t < 0)
            t_hit[cross], z_at[cross], steps[cross] = t[cross], z_k, k
            done |= cross
            go = live & ok & ~cross
            have_prev[go] = True
            t_prev[go] = t[go]
            z_prev[go] = z_k
        with np.errstate(all="ignore"):
            z_hit = z_prev + (t_prev / (t_prev - t_hit)) * (z_at - z_prev)
        ok, _, c, fr, lin = _sample(tsdf, obs, dims, a, b, z_hit)
        cov = done & ok
        with np.errstate(all="ignore"):
            G = np.stack([_lerp(_lerp(c[1] - c[0], c[3] - c[2], fr[1]), _lerp(c[5] - c[4], c[7] - c[6], fr[1]), fr[2]),
                          _lerp(_lerp(c[2] - c[0], c[3] - c[1], fr[0]), _lerp(c[6] - c[4], c[7] - c[5], fr[0]), fr[2]),
                          _lerp(_lerp(c[4] - c[0], c[5] - c[1], fr[0]), _lerp(c[6] - c[2], c[7] - c[3], fr[0]), fr[1])])
        near = np.where(cov, lin + (fr[0] >= F(0.5)) + (fr[1] >= F(0.5)) * Nx + (fr[2] >= F(0.5)) * Nx * Ny, 0)
        byte = ((col[:, near] + 128) >> 8).astype(np.uint8)
        out["depth"][bi, 0] = np.where(cov, z_hit, F(0)).reshape(Ht, Wt)
        out["gradients"][bi] = np.where(cov, G, F(0)).reshape(3, Ht, Wt)
        out["image"][bi] = np.where(cov, byte, 0).reshape(3, Ht, Wt)
        out["count"][bi] = cov.sum()
        out["steps"][bi] = steps.reshape(Ht, Wt)
        out["reset"][bi] = (reset & done).reshape(Ht, Wt)
        out["hit_unobserved"][bi] = (done & ~ok).reshape(Ht, Wt)
        out["fr_hit"][bi] = np.where(cov, fr, F(np.nan)).reshape(3, Ht, Wt)
        out["t_prev"][bi] = np.where(done, t_prev, F(np.nan)).reshape(Ht, Wt)
        out["on_centre"][bi] = on_centre.reshape(Ht, Wt)
        out["on_edge"][bi] = on_edge.reshape(Ht, Wt)
    return out
