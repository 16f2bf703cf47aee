"""numpy oracle of the surface mesh stage (K20, include/s2m2_hip.h: s2m2_mesh), independent of the code under test and written from the header's
text, case by case.

The vertices are ``cloud_oracle.cloud``'s: ``mesh`` takes its ``keep`` (H,W) and ``index`` (flat indices of the kept pixels in raster order, so
that the rank of a vertex is its position in that list) plus the cropped disparity MAP (the map's own values, not the filtered ones).

    joined(p, q) = keep(p) && keep(q) && |d_p - d_q| <= max_jump          in float32; a comparison with NaN is false
    quad (v,u): a=(v,u)  b=(v,u+1)  c=(v+1,u)  e=(v+1,u+1)
      four kept:   |d_a - d_e| <= |d_b - d_c|  ->  (a,c,e) then (a,e,b);   otherwise (a,c,b) then (b,c,e)
      three kept:  e missing (a,c,b);  a missing (b,c,e);  b missing (a,c,e);  c missing (a,e,b)
      a candidate is emitted iff its three edges are joined
    faces in raster order of their quad, within a quad in the order listed

Everything is array arithmetic over the (H-1, W-1) grid of quads: no per-pixel Python loop.
"""
import numpy as np

F = np.float32
HIST_KEYS = ("kept4_diag_ae", "kept4_diag_bc", "kept4_tie", "kept3_miss_a", "kept3_miss_b", "kept3_miss_c", "kept3_miss_e", "kept_fewer",
             "emit4_ace", "emit4_aeb", "emit4_acb", "emit4_bce", "emit3_acb", "emit3_bce", "emit3_ace", "emit3_aeb", "emit_tie",
             "edge_at_max_jump", "quads_0_faces", "quads_1_face", "quads_2_faces")


def _corners(a):
    """(H,W) -> the four (H-1,W-1) corner views a, b, c, e of every quad"""
    return a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:]


def mesh(keep, index, disp, max_jump=1.0):
    """keep (H,W) bool, index (n) flat kept pixels in raster order, disp (H,W) float32 cropped map.  Returns a dict: faces (m,3) int64 vertex
    ranks, rank (H,W) int64 (-1: not a vertex), hist: how often every branch of the rule occurs (HIST_KEYS)."""
    keep = np.asarray(keep, dtype=bool)
    disp = np.ascontiguousarray(disp, dtype=F)
    H, W = keep.shape
    rank = np.full(H * W, -1, dtype=np.int64)
    rank[np.asarray(index, dtype=np.int64)] = np.arange(len(index), dtype=np.int64)
    rank = rank.reshape(H, W)
    hist = dict.fromkeys(HIST_KEYS, 0)
    if H < 2 or W < 2:
        hist["quads_0_faces"] = 0
        return dict(faces=np.zeros((0, 3), np.int64), rank=rank, hist=hist)
    mj = F(max_jump)
    k, d, r = dict(zip("abce", _corners(keep))), dict(zip("abce", _corners(disp))), dict(zip("abce", _corners(rank)))

    with np.errstate(invalid="ignore", over="ignore"):
        def gap(p, q):
            return np.abs(d[p] - d[q])                   # float32; NaN where either is NaN or both are the same infinity

        def joined(p, q):
            return k[p] & k[q] & (gap(p, q) <= mj)

        def emitted(t):
            return joined(t[0], t[1]) & joined(t[1], t[2]) & joined(t[2], t[0])

        nkept = k["a"].astype(int) + k["b"] + k["c"] + k["e"]
        four = nkept == 4
        ae = four & (gap("a", "e") <= gap("b", "c"))
        bc = four & ~ae
        tie = four & (gap("a", "e") == gap("b", "c"))
        three = nkept == 3
        miss = {c: three & ~k[c] for c in "abce"}
        # (condition, candidates in the order listed)
        rules = [(ae, ("ace", "aeb")), (bc, ("acb", "bce")), (miss["e"], ("acb",)), (miss["a"], ("bce",)), (miss["b"], ("ace",)),
                 (miss["c"], ("aeb",))]
        Hq, Wq = H - 1, W - 1
        tri = np.full((Hq, Wq, 2, 3), -1, dtype=np.int64)
        out = np.zeros((Hq, Wq, 2), dtype=bool)
        for cond, cands in rules:
            for slot, t in enumerate(cands):
                m = cond & emitted(t)
                out[..., slot] |= m
                for i, c in enumerate(t):
                    tri[..., slot, i] = np.where(m, r[c], tri[..., slot, i])
                hist[("emit4_" if len(cands) == 2 else "emit3_") + t] += int(m.sum())
        at_jump = sum(int((k[p] & k[q] & (gap(p, q) == mj)).sum()) for p, q in ("ab", "ac", "ae", "bc"))
        # (ab and ac over all quads miss the last row's horizontal and the last column's vertical edges: count those too)
        at_jump += int((keep[-1, :-1] & keep[-1, 1:] & (np.abs(disp[-1, :-1] - disp[-1, 1:]) == mj)).sum())
        at_jump += int((keep[:-1, -1] & keep[1:, -1] & (np.abs(disp[:-1, -1] - disp[1:, -1]) == mj)).sum())
    per_quad = out.sum(axis=2)
    hist.update(kept4_diag_ae=int(ae.sum()), kept4_diag_bc=int(bc.sum()), kept4_tie=int(tie.sum()), kept_fewer=int((nkept < 3).sum()),
                emit_tie=int((tie & (per_quad > 0)).sum()), edge_at_max_jump=at_jump, quads_0_faces=int((per_quad == 0).sum()),
                quads_1_face=int((per_quad == 1).sum()), quads_2_faces=int((per_quad == 2).sum()),
                **{f"kept3_miss_{c}": int(miss[c].sum()) for c in "abce"})
    faces = tri[out]                                     # boolean indexing walks (v, u, slot) in C order: raster order, then the order listed
    assert faces.shape[1] == 3 and (faces >= 0).all()
    return dict(faces=faces, rank=rank, hist=hist)
