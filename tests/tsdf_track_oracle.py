"""numpy oracle of K27 (include/s2m2_hip.h: s2m2_tsdf_track), independent of the code under test.

The per-pixel rule of the header restated with float32 ARRAY arithmetic -- every elementwise numpy operation on float32 arrays is one IEEE
rounding, and nothing is fused --, vectorised over the pixels of one pair; keep and z of a pixel come from cloud_oracle (K15's).  The 28 sums
are math.fsum over the exact double products (a product of two widened float32 values has 48 significant bits), i.e. the exact sums rounded
once; beside each the oracle returns sum |term| and the count, from which the tests bound ANY order of additions.  Solve and update in float64.
"""
import math

import numpy as np

import cloud_oracle

F = np.float32
HOLE_BITS = 0x7fc00000
U = 2.0 ** -53

# what happened to a live pixel (iterate's `cls`): the skip reasons of the header in their order, then USED
NOT_KEPT, BEHIND, OUTSIDE, MODEL_HOLE, ZERO_GRADIENT, FAR, USED = range(7)


def gamma(k):
    """gamma_k = k u / (1 - k u): the bound of k roundings (Higham)"""
    return k * U / (1.0 - k * U)


def rows(disp, occ, conf, pose, mpose, mdepth, mgrad, *, H, W, fx, fy, cx, cy, mfx, mfy, mcx, mcy, max_dist, **cam):
    """One pair.  disp / occ / conf (Hp,Wp) float32 PADDED; pose, mpose (12); mdepth (Ht,Wt), mgrad (3,Ht,Wt).  cam: the remaining keywords of
    cloud_oracle.cloud.  -> cls (H*W) int8, J (H*W, 6) float32, r (H*W) float32 (both meaningful where cls == USED)"""
    c = cloud_oracle.cloud(cloud_oracle.crop(disp, H, W), cloud_oracle.crop(occ, H, W), cloud_oracle.crop(conf, H, W),
                           np.zeros((3, H, W), np.uint8), fx=fx, fy=fy, cx=cx, cy=cy, **cam)
    keep = c["keep"].ravel()
    z = c["depth"].ravel().astype(F)
    v, u = (a.ravel() for a in np.mgrid[0:H, 0:W])
    q, m = np.asarray(pose, F), np.asarray(mpose, F)
    Ht, Wt = mdepth.shape
    md, mg = np.asarray(mdepth, F).ravel(), np.asarray(mgrad, F).reshape(3, -1)
    md2 = F(max_dist) * F(max_dist)
    with np.errstate(all="ignore"):
        x = (u.astype(F) - F(cx)) * z / F(fx)
        y = (v.astype(F) - F(cy)) * z / F(fy)
        c0, c1, c2 = x - q[3], y - q[7], z - q[11]
        p = [(q[a] * c0 + q[4 + a] * c1) + q[8 + a] * c2 for a in range(3)]
        X = ((m[0] * p[0] + m[1] * p[1]) + m[2] * p[2]) + m[3]
        Y = ((m[4] * p[0] + m[5] * p[1]) + m[6] * p[2]) + m[7]
        Z = ((m[8] * p[0] + m[9] * p[1]) + m[10] * p[2]) + m[11]
        front = keep & (Z > 0) & np.isfinite(Z)
        up = (F(mfx) * X) / Z + F(mcx)
        vp = (F(mfy) * Y) / Z + F(mcy)
        fu, fv = np.rint(up), np.rint(vp)
        inside = front & (fu >= 0) & (fu < F(Wt)) & (fv >= 0) & (fv < F(Ht))
        pix = np.where(inside, fv, 0).astype(np.int64) * Wt + np.where(inside, fu, 0).astype(np.int64)
        dm = md[pix]
        surf = inside & (dm > 0)
        gx, gy, gz = mg[0][pix], mg[1][pix], mg[2][pix]
        s = (gx * gx + gy * gy) + gz * gz
        grad = surf & (s > 0) & np.isfinite(s)
        ln = np.sqrt(s)
        n = [gx / ln, gy / ln, gz / ln]
        mx = (fu - F(mcx)) * dm / F(mfx)
        my = (fv - F(mcy)) * dm / F(mfy)
        e0, e1, e2 = mx - m[3], my - m[7], dm - m[11]
        w = [(m[a] * e0 + m[4 + a] * e1) + m[8 + a] * e2 for a in range(3)]
        d = [w[a] - p[a] for a in range(3)]
        used = grad & ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= md2)
        r = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]
        J = np.stack([p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]], 1)
    cls = np.full(H * W, NOT_KEPT, np.int8)
    cls[keep] = BEHIND
    cls[front] = OUTSIDE
    cls[inside] = MODEL_HOLE
    cls[surf] = ZERO_GRADIENT
    cls[grad] = FAR
    cls[used] = USED
    assert J.dtype == F and r.dtype == F
    return cls, J, r


def sums(J, r):
    """J (n,6), r (n) float32 of the used pixels -> exact-rounded sums (28) and sum |term| (28), in the order of a `systems` row"""
    Jd = np.concatenate([J.astype(np.float64), r.astype(np.float64)[:, None]], 1)
    pairs = [(i, j) for i in range(6) for j in range(i, 6)] + [(i, 6) for i in range(7)]
    s, a = np.zeros(28), np.zeros(28)
    for k, (i, j) in enumerate(pairs):
        t = Jd[:, i] * Jd[:, j]                          # exact
        s[k], a[k] = math.fsum(t), math.fsum(np.abs(t))
    return s, a


def sum_errors(J, r, got):
    """|exact sum - got[k]| for the 28 sums, each rounded once (math.fsum over the exact terms and -got[k]): what the tests hold against
    gamma_{n-1} * sum |term|"""
    Jd = np.concatenate([J.astype(np.float64), r.astype(np.float64)[:, None]], 1)
    pairs = [(i, j) for i in range(6) for j in range(i, 6)] + [(i, 6) for i in range(7)]
    return np.array([abs(math.fsum(list(Jd[:, i] * Jd[:, j]) + [-float(got[k])])) for k, (i, j) in enumerate(pairs)])


def _sym(tri):
    A = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = tri[k]
            k += 1
    return A


def _cholesky_solve(A, b):
    """-> xi, or None at a pivot that is not > 0 (or not finite)"""
    L = np.zeros((6, 6))
    for j in range(6):
        d = A[j, j] - float(np.dot(L[j, :j], L[j, :j]))
        if not (d > 0.0 and math.isfinite(d)):
            return None
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - float(np.dot(L[i, :j], L[j, :j]))) / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (b[i] - float(np.dot(L[i, :i], y[:i]))) / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = (y[i] - float(np.dot(L[i + 1:, i], x[i + 1:]))) / L[i, i]
    return x


def rodrigues(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    if th < 1e-4:
        a, b = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        a, b = math.sin(th) / th, (1.0 - math.cos(th)) / (th * th)
    return np.eye(3) + a * K + b * (K @ K)


def update(pose, xi):
    """pose (12) float32, xi (6) float64 -> the new pose (12) float64, unrounded"""
    P = np.asarray(pose, np.float64).reshape(3, 4)
    R = P[:, :3] @ rodrigues(xi[:3]).T
    r0 = R[0] / np.linalg.norm(R[0])
    r1 = R[1] - np.dot(r0, R[1]) * r0
    r1 = r1 / np.linalg.norm(r1)
    R = np.stack([r0, r1, np.cross(r0, r1)])
    t = P[:, 3] - R @ xi[3:]
    return np.concatenate([R, t[:, None]], 1).ravel()


def solve(s, a, count, pose, *, min_count, max_rot, max_trans):
    """the verdict and the update from the sums -> dict: status, wn, vn, P (12 float64, unrounded; the old pose unless status 0), pose (12)
    float32, kappa and bound: with status 0 the bound of the change of any entry of P under ANY order of the additions (see pose_bound)"""
    old = np.asarray(pose, F)
    out = dict(status=0, wn=0.0, vn=0.0, P=old.astype(np.float64), pose=old.copy(), kappa=math.inf, bound=math.inf, xi=np.zeros(6))
    if count < min_count:
        out["status"] = 1
        return out
    if not np.isfinite(s).all():
        out["status"] = 2
        return out
    A, b = _sym(s[:21]), s[21:27]
    with np.errstate(all="ignore"):
        xi = _cholesky_solve(A, b)
    if xi is None or not np.isfinite(xi).all():
        out["status"] = 2
        return out
    wn, vn = float(np.linalg.norm(xi[:3])), float(np.linalg.norm(xi[3:]))
    if wn > max_rot or vn > max_trans:
        out.update(status=3, wn=wn, vn=vn)
        return out
    with np.errstate(all="ignore"):
        P = update(old, xi)
        P32 = P.astype(F)
    if not np.isfinite(P32).all():
        out["status"] = 2
        return out
    out.update(wn=wn, vn=vn, P=P, pose=P32, xi=xi, kappa=float(np.linalg.cond(A)))
    out["bound"] = pose_bound(A, b, xi, _sym(a[:21]), a[21:27], count, old)
    return out


def pose_bound(A, b, xi, absA, absb, count, pose):
    """How far an entry of the unrounded new pose may move when the sums are formed in another order and the 6 x 6 system is solved by another
    backward-stable method in double.  k = count + 100 roundings: count - 1 for the additions of a sum (any order: |dA_ij| <= gamma_k *
    sum |term|), the rest for the Cholesky factorisation and the two triangular solves of a 6 x 6 system on either side (backward errors of
    a few dozen u).  The standard bound of a perturbed linear system,
        |d xi| <= kappa_2(A) * (|dA| / |A| + |db| / |b|) * |xi|            (first order; the factor 2 below covers the second),
    with |dA|_2 <= |dA|_F <= gamma_k |absA|_F and |db|_2 <= gamma_k |absb|_2, is carried through the update: Rodrigues' formula is
    1-Lipschitz in omega, the re-orthonormalisation of nearly orthonormal rows at most triples a perturbation, and t' = t - R' v adds
    |dR'| |v| + |R'| |dv|; the update's own few dozen roundings in double are covered by 100 u (1 + |t|)."""
    g = gamma(count + 100)
    kappa = float(np.linalg.cond(A))
    nb = float(np.linalg.norm(b))
    rel = g * float(np.linalg.norm(absA)) / float(np.linalg.norm(A, 2)) + (g * float(np.linalg.norm(absb)) / nb if nb > 0 else 0.0)
    dxi = 2.0 * kappa * rel * float(np.linalg.norm(xi)) + g * float(np.linalg.norm(absb)) * kappa / float(np.linalg.norm(A, 2)) * (nb == 0)
    P = np.asarray(pose, np.float64).reshape(3, 4)
    nR = float(np.linalg.norm(P[:, :3], 2))
    dR = 3.0 * nR * dxi
    dt = dR * float(np.linalg.norm(xi[3:])) + 1.5 * nR * dxi
    return max(dR, dt) + 100.0 * U * (1.0 + float(np.abs(P).max()))


def iterate(disp, occ, conf, pose, mpose, mdepth, mgrad, *, min_count, max_rot, max_trans, **kw):
    """one iteration of one pair -> solve()'s dict plus cls (H,W), residual (H,W) float32 with HOLE_BITS where no correspondence, sums,
    abs (28 each), count, row (32 float64: the `systems` row), J (count, 6) and r (count) float32 of the used pixels in raster order"""
    H, W = kw["H"], kw["W"]
    cls, J, r = rows(disp, occ, conf, pose, mpose, mdepth, mgrad, **kw)
    used = cls == USED
    s, a = sums(J[used], r[used])
    count = int(used.sum())
    out = solve(s, a, count, pose, min_count=min_count, max_rot=max_rot, max_trans=max_trans)
    res = np.full(H * W, HOLE_BITS, np.uint32)
    res[used] = r[used].view(np.uint32)
    row = np.zeros(32)
    row[:28], row[28], row[29], row[30], row[31] = s, count, out["status"], out["wn"], out["vn"]
    out.update(cls=cls.reshape(H, W), residual=res.view(F).reshape(H, W), sums=s, abs=a, count=count, row=row, J=J[used], r=r[used])
    return out


def track(disp, occ, conf, poses, mposes, mdepth, mgrad, *, n_iters, **kw):
    """disp / occ / conf (B,Hp,Wp); poses, mposes (B,12); mdepth (B,1,Ht,Wt); mgrad (B,3,Ht,Wt) -> dict: poses (B,12) float32, systems
    (B,n_iters,32), residual (B,1,H,W) of the last iteration, its (B x n_iters) list of iterate()'s dicts"""
    B = len(poses)
    H, W = kw["H"], kw["W"]
    out = dict(poses=np.array(poses, F), systems=np.zeros((B, n_iters, 32)), residual=np.zeros((B, 1, H, W), F), its=[])
    for b in range(B):
        its = []
        for it in range(n_iters):
            o = iterate(disp[b], occ[b], conf[b], out["poses"][b], mposes[b], mdepth[b, 0], mgrad[b], **kw)
            out["poses"][b] = o["pose"]
            out["systems"][b, it] = o["row"]
            its.append(o)
        out["residual"][b, 0] = its[-1]["residual"]
        out["its"].append(its)
    return out


def pose_errors(pose, truth):
    """rotation angle (rad) and translation distance between two world -> camera poses (12 each), compared as camera-to-world motions"""
    P, T = np.asarray(pose, np.float64).reshape(3, 4), np.asarray(truth, np.float64).reshape(3, 4)
    dR = P[:, :3] @ T[:, :3].T
    ang = math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1.0) / 2.0)))
    cp, ct = -P[:, :3].T @ P[:, 3], -T[:, :3].T @ T[:, 3]
    return ang, float(np.linalg.norm(cp - ct))
