"""Cases shared by the CPU and GPU tests of K29, on the scenes of normals_cases.py, chosen so that every branch of the rule decides some pixel.
Nothing here computes an expected result: that is smooth_oracle's.  A case is a dict: name, maps = (disp, occ, conf) each (B,Hp,Wp) float32,
kw = the keywords of smooth_oracle.smooth WITHOUT the tables, sigma = (sigma_s, sigma_r) from which the caller forms them (the CPU tests with
smooth_oracle.tables, the GPU tests with the library's s2m2_smooth_weights), classes = the classes of smooth_oracle that the case is meant to
exercise (the CPU test asserts FROM THE ORACLE that each has members).  Everything is computed once per process."""
import functools

import numpy as np

import normals_cases as NC
import smooth_oracle as O
import tsdf_track_scenes as TS

F = np.float32
RADII = (1, 2, 3, 5, 8)


def _case(name, maps, kw, classes, *, radius, sigma_r, max_jump, sigma_s=None):
    maps = tuple(np.ascontiguousarray(m if m.ndim == 3 else m[None], dtype=F) for m in maps)
    return dict(name=name, maps=maps, kw=dict(kw, radius=radius, max_jump=max_jump), sigma=(radius / 2.0 if sigma_s is None else sigma_s, sigma_r),
                classes=tuple(classes))


def edge_scene(noise=True):
    """the curved scene with a one-metre step at column 45 (disparities 0.44 .. 1.12 px), unpadded, and Gaussian disparity noise of 0.02 px"""
    z = TS.curved_depth(45, 67)
    z[:, 45:] -= 1.0
    disp, occ, conf = TS.pad(z, 45, 67)
    if noise:
        disp = disp + np.random.default_rng(3).normal(0, 0.02, disp.shape).astype(F)
    return (disp.astype(F), occ, conf), dict(NC.CAM, H=45, W=67, cx=33.0, cy=22.0)


EDGE = dict(radius=3, sigma_s=2.0, sigma_r=0.06)


@functools.lru_cache(None)
def cases():
    K, A, G, U = O.NOT_KEPT, O.ALONE, O.GATED, O.FULL
    out = []
    # the tracking scenes: smooth surfaces in padding that holds KEPT pixels 0.07 px away from the surface (inside the gate: a kernel that
    # read them would average them in)
    std = dict(sigma_r=0.03, max_jump=0.25)
    maps, kw = NC._frame("own", 51, 73)
    for r in RADII:
        out.append(_case(f"own_r{r}", maps, kw, (U,), radius=r, **std))
    maps, kw = NC._frame("big", 98, 140)
    out.append(_case("big_padded_r2", maps, kw, (U,), radius=2, **std))
    out.append(_case("big_padded_r8", maps, kw, (U,), radius=8, **std))
    maps, kw = NC._frame("big", 92, 134)                     # Wp % 4 == 2: the per-pixel loads
    out.append(_case("big_unpadded_r5", maps, kw, (U,), radius=5, **std))
    maps, kw = NC._frame("row", 7, 73)
    out.append(_case("row_r3", maps, kw, (U,), radius=3, **std))
    maps, kw = NC._frame("col", 51, 7)
    out.append(_case("col_r2", maps, kw, (U,), radius=2, **std))
    small = dict(NC.CAM, H=5, W=3, cx=1.0, cy=2.0)
    tiny = TS.pad(TS.curved_depth(5, 3), 9, 7)
    out.append(_case("5x3_r1", tiny, small, (U,), radius=1, **std))
    out.append(_case("5x3_r8", tiny, small, (U,), radius=8, **std))
    low = dict(NC.CAM, H=7, W=40, cx=19.5, cy=3.0)
    out.append(_case("r8_seven_rows", TS.pad(TS.curved_depth(7, 40), 11, 44), low, (U,), radius=8, **std))
    # the two steps with one-pixel ridges: 0.01 px per column, 0.005 px per row, steps of 8 px
    st = dict(NC.CAM, H=24, W=40, cx=19.5, cy=11.5)
    steps = NC._from_disp(NC.step_disp(), 30, 48, 0.5)
    out.append(_case("steps_r2", steps, st, (U, G), radius=2, sigma_r=0.02, max_jump=1.0))
    out.append(_case("steps_r5", steps, st, (G,), radius=5, sigma_r=0.02, max_jump=1.0))
    out.append(_case("steps_joined", steps, st, (U,), radius=2, sigma_r=0.02, max_jump=float("inf")))      # 8 px >> 4 sigma_r: the clamp at 256
    out.append(_case("steps_gate0", steps, st, (A,), radius=1, sigma_r=0.02, max_jump=0.0))
    # non-finite and filtered blocks, with and without the filter
    maps, kw = NC._frame("own", 51, 73)
    bad = NC.spoiled(maps)
    out.append(_case("spoiled", bad, kw, (U, K, G), radius=2, **std))
    out.append(_case("spoiled_unfiltered", bad, dict(kw, filtered=False), (U, K, G), radius=3, **std))
    # two pairs with different maps
    both = tuple(np.stack([a, b]) for a, b in zip(maps, TS.plane_live(51, 73)))
    out.append(_case("two_pairs", both, kw, (U,), radius=3, **std))
    # the noisy edge: the gate below the step (nothing crosses it) and above it (the range weight alone holds the edge)
    emaps, ekw = edge_scene()
    out.append(_case("edge", emaps, ekw, (U, G), max_jump=0.25, **EDGE))
    out.append(_case("edge_open", emaps, ekw, (U,), max_jump=1.0, **EDGE))
    # ... and a gate of two sigma of the noise: it decides inside the surfaces too, so WHAT it is taken against matters
    out.append(_case("edge_tight", emaps, ekw, (U, G), radius=2, sigma_r=0.03, max_jump=0.04))
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def oracle(c, tables, **wrong):
    """smooth_oracle.batch on the case c with the tables from `tables(radius, sigma_s, sigma_r)` -> (ws, wr, inv)"""
    ws, wr, inv = tables(c["kw"]["radius"], *c["sigma"])
    return O.batch(*c["maps"], **c["kw"], ws=ws, wr=wr, inv=inv, **wrong)
