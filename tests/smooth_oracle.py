"""numpy oracle of K29 (include/s2m2_hip.h: s2m2_smooth), independent of the code under test.

The per-pixel rule of the header restated with float32 ARRAY arithmetic -- every elementwise numpy operation on float32 arrays is one IEEE
rounding, and nothing is fused --, vectorised over the pixels of one pair: the window is walked in the rule's raster order, one shifted copy of
the map per tap, so that the additions of every pixel happen in the rule's order.  keep comes from cloud_oracle (K15's), on the CROPPED maps,
so a padded pixel can never be a neighbour.  The division of float32 arrays is correctly rounded, as the rule requires of the kernel; np.fmin
returns the number when one operand is a NaN, as fminf does.  The weight tables are ARGUMENTS: the GPU tests pass the library's own
(s2m2_smooth_weights), the CPU tests those of ``tables``.  ``smooth`` takes the switches of the wrong kernels of test_smooth_cpu.py; all of
them default to the rule.
"""
import numpy as np

import cloud_oracle

F = np.float32
RANGE = 256

# what happened to a pixel
NOT_KEPT, ALONE, GATED, FULL = range(4)
CLASS_NAMES = ("not kept", "alone (taps == 1)", "gated (a kept neighbour failed max_jump)", "full")


def tables(radius, sigma_s, sigma_r):
    """the header's tables in float64, each entry rounded once to float32 -> (ws (9,), entries behind radius 0; wr (257,); inv)"""
    k = np.arange(9, dtype=np.float64)
    ws = np.where(k <= radius, np.exp(-(k * k) / (2.0 * float(sigma_s) ** 2)), 0.0).astype(F)
    e = np.arange(RANGE + 1, dtype=np.float64) * (4.0 * float(sigma_r) / RANGE)
    wr = np.exp(-(e * e) / (2.0 * float(sigma_r) ** 2)).astype(F)
    return ws, wr, F(RANGE / (4.0 * float(sigma_r)))


def _shift(a, dv, du, fill):
    """out[v, u] = a[v + dv, u + du] where that lies inside the array, else fill"""
    H, W = a.shape
    out = np.full_like(a, fill)
    v0, v1, u0, u1 = max(0, -dv), min(H, H - dv), max(0, -du), min(W, W - du)
    if v0 < v1 and u0 < u1:
        out[v0:v1, u0:u1] = a[v0 + dv:v1 + dv, u0 + du:u1 + du]
    return out


def smooth(disp, occ, conf, *, H, W, radius, max_jump, ws, wr, inv, jump_scaled=False, gate_running_mean=False, index_rounded=False,
           no_clamp=False, column_major=False, ws_of_sum=False, no_crop=False, padded_neighbours=False, mean_of_dq=False, radius_one=False,
           **cam):
    """One pair.  disp / occ / conf (Hp,Wp) float32 PADDED; ws (9,), wr (257,) float32 and inv: the tables; cam: the keywords of
    cloud_oracle.cloud (fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min, occ_min, filtered).  -> dict: disp_out (Hp,Wp)
    float32, taps (H,W) int32, count, cls (H,W) int8.  The keywords behind inv are the WRONG kernels of the CPU test."""
    Hp, Wp = disp.shape
    ws, wr, inv = np.asarray(ws, F), np.asarray(wr, F), F(inv)
    assert ws.shape == (9,) and wr.shape == (RANGE + 1,)
    ry, rx = (Hp - H) // 2, (Wp - W) // 2                    # where the result goes in the padded map
    if padded_neighbours:                                    # evaluate the whole padded map and crop the RESULT: the border becomes a neighbour
        full = smooth(disp, occ, conf, H=Hp, W=Wp, radius=radius, max_jump=max_jump, ws=ws, wr=wr, inv=inv, **cam)
        out = np.full((Hp, Wp), F(-1))
        out[ry:ry + H, rx:rx + W] = full["disp_out"][ry:ry + H, rx:rx + W]
        taps = np.ascontiguousarray(full["taps"][ry:ry + H, rx:rx + W])
        cls = np.ascontiguousarray(full["cls"][ry:ry + H, rx:rx + W])
        return dict(disp_out=out, taps=taps, count=int((cls != NOT_KEPT).sum()), cls=cls)
    oy, ox = (0, 0) if no_crop else (ry, rx)
    r = 1 if radius_one else int(radius)
    win = lambda m: np.ascontiguousarray(np.asarray(m, F)[oy:oy + H, ox:ox + W])
    d = win(disp)
    keep = cloud_oracle.cloud(d, win(occ), win(conf), np.zeros((3, H, W), np.uint8), **cam)["keep"]
    gate = F(max_jump) * F(radius) if jump_scaled else F(max_jump)
    num, den, n = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), np.int32)
    failed = np.zeros((H, W), bool)                          # some kept in-image neighbour failed the gate
    window = [(dv, du) for dv in range(-r, r + 1) for du in range(-r, r + 1)]
    if column_major:                                         # WRONG: du outer, dv inner
        window = [(dv, du) for du in range(-r, r + 1) for dv in range(-r, r + 1)]
    with np.errstate(all="ignore"):
        for dv, du in window:
            kq, dq = _shift(keep, dv, du, False), _shift(d, dv, du, F(0))
            e = dq - d
            a = np.abs(e)
            if gate_running_mean:                            # WRONG: the gate against the mean so far
                mean = np.where(den > 0, d + num / den, d)
                ok = np.abs(dq - mean) <= gate
            else:
                ok = a <= gate
            t = a * inv
            if not no_clamp:
                t = np.fmin(t, F(RANGE))
            t = np.fmin(np.where(np.isfinite(t), t, F(RANGE)), F(1e9))     # (only without the clamp is t anything but a number in [0, 256])
            i = (np.rint(t) if index_rounded else t).astype(np.int64)      # WRONG: rounded;  the rule truncates
            wi = np.where(i <= RANGE, wr[np.minimum(i, RANGE)], F(0))      # (WRONG, no clamp: beyond the table the weight is 0)
            wsp = ws[min(abs(dv) + abs(du), 8)] if ws_of_sum else ws[abs(dv)] * ws[abs(du)]
            w = F(wsp) * wi
            enters = keep & kq & ok
            term = w * (dq if mean_of_dq else e)
            num = np.where(enters, num + term, num)
            den = np.where(enters, den + w, den)
            n = n + enters
            failed |= keep & kq & ~ok
        assert num.dtype == F and den.dtype == F and w.dtype == F
        q = num / den
        res = q if mean_of_dq else d + q                     # WRONG: the weighted mean of d_q itself
    assert res.dtype == F
    out = np.full((Hp, Wp), F(-1))
    out[ry:ry + H, rx:rx + W] = np.where(keep, res, F(-1))
    taps = np.where(keep, n, 0).astype(np.int32)
    cls = np.full((H, W), NOT_KEPT, np.int8)
    cls[keep] = FULL
    cls[keep & failed] = GATED
    cls[keep & (taps == 1)] = ALONE
    return dict(disp_out=out, taps=taps, count=int(keep.sum()), cls=cls)


def batch(disp, occ, conf, **kw):
    """disp / occ / conf (B,Hp,Wp) -> dict: disp_out (B,1,Hp,Wp), taps (B,1,H,W), count (B) int32, cls (B,H,W)"""
    outs = [smooth(disp[b], occ[b], conf[b], **kw) for b in range(len(disp))]
    return dict(disp_out=np.stack([o["disp_out"] for o in outs])[:, None], taps=np.stack([o["taps"] for o in outs])[:, None],
                count=np.array([o["count"] for o in outs], np.int32), cls=np.stack([o["cls"] for o in outs]))
