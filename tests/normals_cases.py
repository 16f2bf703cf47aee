"""Cases shared by the CPU and GPU tests of K28, chosen so that every branch of the rule decides some pixel.  Nothing here computes an expected
result: that is normals_oracle's.  A case is a dict: name, maps = (disp, occ, conf) each (B,Hp,Wp) float32, kw = the keywords of
normals_oracle.normals, classes = the classes of normals_oracle that the case is meant to exercise (the CPU test asserts FROM THE ORACLE that
each has members).  Everything is computed once per process."""
import functools

import numpy as np

import normals_oracle as N
import tsdf_scenes as S
import tsdf_track_scenes as TS

F = np.float32
CAM = {k: TS.CAM_LIVE[k] for k in ("fx", "fy", "cx", "cy", "baseline", "doffs", "depth_scale", "depth_trunc", "conf_min", "occ_min")}


def _case(name, maps, kw, classes, **rule):
    maps = tuple(np.ascontiguousarray(m if m.ndim == 3 else m[None], dtype=F) for m in maps)
    return dict(name=name, maps=maps, kw=dict(kw, **rule), classes=tuple(classes))


def _frame(cam, Hp, Wp):
    """the tracking scenes' previous frame: the model seen from the identity, in padding that holds KEPT pixels"""
    return TS.live(cam, Hp, Wp, pose=tuple(S.IDENTITY))


def _from_disp(disp, Hp, Wp, border):
    """(H,W) disparity -> padded maps with a KEPT border of disparity `border`"""
    H, W = disp.shape
    oy, ox = (Hp - H) // 2, (Wp - W) // 2
    full = np.full((Hp, Wp), border, F)
    full[oy:oy + H, ox:ox + W] = disp
    return full, np.ones((Hp, Wp), F), np.ones((Hp, Wp), F)


def step_disp(H=24, W=40):
    """a gently sloped map with two disparity steps of more than any gate used here, a ridge ONE pixel wide between them (column 15), and a
    second ridge one pixel high (row 9, columns 25..39)"""
    v, u = np.mgrid[0:H, 0:W]
    d = (0.5 + 0.01 * u + 0.005 * v).astype(F)
    d[:, 15] += F(8.0)
    d[:, 16:] += F(16.0)
    d[9, 25:] += F(8.0)
    return d


def tilted_disp(H=24, W=40):
    """a steeply tilted plane: 0.3 px of disparity per column, so that neighbours three columns away differ by 0.9 px"""
    v, u = np.mgrid[0:H, 0:W]
    return (2.0 + 0.3 * u + 0.01 * v).astype(F)


def spoiled(maps):
    """blocks of disp 0, negative, NaN, +Inf and 1e30 (kept at z = 1e-30: the cross product underflows to 0), of conf and occ below the
    thresholds"""
    disp, occ, conf = (m.copy() for m in maps)
    disp[8:12, 10:16] = 0.0
    disp[8:12, 20:26] = -1.5
    disp[8:12, 30:36] = np.nan
    disp[8:12, 40:46] = np.inf
    disp[30:36, 40:48] = 1e30
    conf[20:24, 10:16] = 0.05
    occ[20:24, 20:26] = 0.25
    conf[20:24, 30:36] = np.nan
    return disp, occ, conf


@functools.lru_cache(None)
def cases():
    U, K, H_, V_, D, G = N.USED, N.NOT_KEPT, N.NO_HORIZONTAL, N.NO_VERTICAL, N.DEGENERATE, N.GRAZING
    out = []
    track = dict(radius=1, max_jump=1.0, min_cos=0.2)
    maps, kw = _frame("own", 51, 73)
    out.append(_case("own", maps, kw, (U,), **track))
    out.append(_case("own_r3", maps, kw, (U,), radius=3, max_jump=1.0, min_cos=0.0))
    maps, kw = _frame("big", 98, 140)
    out.append(_case("big_padded", maps, kw, (U,), **track))
    maps, kw = _frame("big", 92, 134)
    out.append(_case("big_unpadded_r2", maps, kw, (U,), radius=2, max_jump=1.0, min_cos=0.2))
    maps, kw = _frame("row", 7, 73)
    out.append(_case("row", maps, kw, (V_,), **track))
    maps, kw = _frame("col", 51, 7)
    out.append(_case("col", maps, kw, (H_,), **track))
    small = dict(CAM, H=5, W=3, cx=1.0, cy=2.0)
    out.append(_case("5x3", TS.pad(TS.curved_depth(5, 3), 9, 7), small, (U,), **track))
    # the steps: one-sided differences next to them, a ridge without a usable horizontal / vertical neighbour
    st = dict(CAM, H=24, W=40, cx=19.5, cy=11.5)
    steps = _from_disp(step_disp(), 30, 48, 0.5)
    out.append(_case("steps", steps, st, (U, H_, V_), radius=1, max_jump=1.0, min_cos=0.0))
    out.append(_case("steps_r2", steps, st, (U, H_, V_), radius=2, max_jump=1.0, min_cos=0.0))
    out.append(_case("steps_joined", steps, st, (U,), radius=1, max_jump=float("inf"), min_cos=0.0))
    out.append(_case("steps_gate0", steps, st, (H_,), radius=1, max_jump=0.0, min_cos=0.0))
    # non-finite and filtered blocks, with and without the filter
    maps, kw = _frame("own", 51, 73)
    bad = spoiled(maps)
    out.append(_case("spoiled", bad, kw, (U, K, D), **track))
    out.append(_case("spoiled_unfiltered", bad, dict(kw, filtered=False), (U, K, D), **track))
    # radius 8 on seven rows: no vertical neighbour anywhere
    low = dict(CAM, H=7, W=40, cx=19.5, cy=3.0)
    out.append(_case("r8_seven_rows", TS.pad(TS.curved_depth(7, 40), 11, 44), low, (V_,), radius=8, max_jump=1.0, min_cos=0.0))
    out.append(_case("r8", _frame("own", 51, 73)[0], _frame("own", 51, 73)[1], (U,), radius=8, max_jump=1.0, min_cos=0.0))
    # the steeply tilted plane against the view gate: kept, split, dropped; its disparity differs by 0.9 px over three columns
    tilt = _from_disp(tilted_disp(), 30, 48, 0.5)
    for mc, cl in ((0.0, (U,)), (0.5, (U, G)), (0.9, (G,))):
        out.append(_case(f"tilted_cos{mc}", tilt, st, cl, radius=3, max_jump=0.35, min_cos=mc))
    # the dyadic plane z = 2: every normal is (0, 0, -1) exactly
    out.append(_case("dyadic_plane", TS.plane_live(51, 73), TS.live()[1], (U,), **track))
    # two pairs with different maps
    own = _frame("own", 51, 73)
    both = tuple(np.stack([a, b]) for a, b in zip(own[0], TS.plane_live(51, 73)))
    out.append(_case("two_pairs", both, own[1], (U,), **track))
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c["name"] == name)
