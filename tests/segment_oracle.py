"""numpy oracle of the connected-component stage (K22, include/s2m2_hip.h: s2m2_segment), independent of the code under test and written from
the header's text.

``keep`` is ``cloud_oracle.cloud``'s chain; the disparity of the rule is the cropped MAP (its own values, not the filtered ones).

    joined(p, q) = keep(p) && keep(q) && |d_p - d_q| <= max_jump      float32, p and q neighbours in a row or in a column
    component    = a class of the transitive closure of joined over the kept pixels
    label        = the smallest raster index of the component (-1: not kept);  size = its pixels (0: not kept)
    survive      = keep && size >= min_size

Components by min-label propagation with pointer jumping: every sweep gives both ends of every joined edge the smaller of their labels, then
replaces every label by its label's label until that changes nothing; the sweeps stop when one changes nothing.  A label only ever decreases,
names a pixel of the same component and is at most the pixel's own index, so the fixed point is the component's minimum.  Array arithmetic
only: a 200x330 percolation mask takes about 130 sweeps and a fraction of a second.
"""
import numpy as np

import cloud_oracle

F = np.float32


def joined_edges(keep, disp, max_jump):
    """(H,W-1) bool: pixel (v,u) joined with (v,u+1); (H-1,W) bool: (v,u) joined with (v+1,u)"""
    keep = np.asarray(keep, dtype=bool)
    d = np.ascontiguousarray(disp, dtype=F)
    mj = F(max_jump)
    with np.errstate(invalid="ignore", over="ignore"):
        jh = keep[:, :-1] & keep[:, 1:] & (np.abs(d[:, :-1] - d[:, 1:]) <= mj)
        jv = keep[:-1, :] & keep[1:, :] & (np.abs(d[:-1, :] - d[1:, :]) <= mj)
    return jh, jv


def components(keep, disp, max_jump=1.0):
    """keep (H,W) bool, disp (H,W) float32 cropped map -> (label (H,W) int32, size (H,W) int32, sweeps)"""
    keep = np.asarray(keep, dtype=bool)
    H, W = keep.shape
    jh, jv = joined_edges(keep, disp, max_jump)
    lab = np.where(keep, np.arange(H * W, dtype=np.int64).reshape(H, W), H * W)
    flat, k = lab.reshape(-1), keep.reshape(-1)              # (views)
    sweeps = 0
    while True:
        before = lab.copy()
        m = np.where(jh, np.minimum(lab[:, :-1], lab[:, 1:]), H * W)        # per edge; a pixel takes the minimum over its edges and itself
        lab[:, :-1] = np.minimum(lab[:, :-1], m)
        lab[:, 1:] = np.minimum(lab[:, 1:], m)
        m = np.where(jv, np.minimum(lab[:-1, :], lab[1:, :]), H * W)
        lab[:-1, :] = np.minimum(lab[:-1, :], m)
        lab[1:, :] = np.minimum(lab[1:, :], m)
        while True:                                          # pointer jumping
            nxt = flat[flat[k]]
            if np.array_equal(nxt, flat[k]):
                break
            flat[k] = nxt
        sweeps += 1
        if np.array_equal(lab, before):
            break
    count = np.bincount(flat[k], minlength=H * W + 1)
    size = np.where(keep, count[np.minimum(lab, H * W)], 0).astype(np.int32)
    return np.where(keep, lab, -1).astype(np.int32), size, sweeps


def segment(disp, occ, conf, *, fx, fy, cx, cy, baseline, doffs=0.0, depth_scale=1000.0, depth_trunc=None, conf_min=0.1, occ_min=0.5,
            filtered=True, max_jump=1.0, min_size=1):
    """One pair: disp / occ / conf (H,W) float32 ALREADY cropped.  Returns a dict: keep (H,W) bool, label (H,W) int32, size (H,W) int32, mask
    (H,W) uint8, stats (4) int32 (kept pixels, components, surviving pixels, surviving components), sweeps."""
    disp = np.ascontiguousarray(disp, dtype=F)
    H, W = disp.shape
    keep = cloud_oracle.cloud(disp, occ, conf, np.zeros((3, H, W), np.uint8), fx=fx, fy=fy, cx=cx, cy=cy, baseline=baseline, doffs=doffs,
                              depth_scale=depth_scale, depth_trunc=depth_trunc, conf_min=conf_min, occ_min=occ_min, filtered=filtered)["keep"]
    label, size, sweeps = components(keep, disp, max_jump)
    survive = keep & (size >= min_size)
    own = np.arange(H * W, dtype=np.int32).reshape(H, W)
    root = label == own
    stats = np.array([keep.sum(), root.sum(), survive.sum(), (root & survive).sum()], dtype=np.int32)
    return dict(keep=keep, label=label, size=size, mask=survive.astype(np.uint8), stats=stats, sweeps=sweeps)


def disp_out(disp_padded, mask, H, W):
    """the padded output map: disp_padded (Hp,Wp) float32 and mask (H,W) of the centred crop -> the map's own value where mask, -1 elsewhere,
    the border included"""
    disp_padded = np.ascontiguousarray(disp_padded, dtype=F)
    out = np.full_like(disp_padded, F(-1.0))
    win, src = cloud_oracle.crop(out, H, W), cloud_oracle.crop(disp_padded, H, W)
    win[...] = np.where(np.asarray(mask, dtype=bool), src, F(-1.0))
    return out
