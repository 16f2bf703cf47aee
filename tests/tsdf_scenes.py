"""Scenes shared by the CPU and GPU tests of K24: small padded maps with an odd crop offset, a camera whose numbers are powers of two (so that
a plane at z = 2 and a grid with a dyadic voxel size give EXACT ties and band edges), and poses.  Nothing here computes an expected result:
that is tsdf_oracle's."""
import numpy as np

F = np.float32
H, W = 45, 67

# z = (baseline * fx / d) / depth_scale = 1 / d: d = 0.5 is z = 2 exactly
CAM = dict(fx=64.0, fy=64.0, cx=33.5, cy=22.5, baseline=1.0, doffs=0.0, depth_scale=64.0, depth_trunc=10.0, conf_min=0.1, occ_min=0.5)

IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


def rot_xy(ax, ay, t):
    """rotation about x by ax, then about y by ay, and a translation -> 12 numbers"""
    cx_, sx, cy_, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    R = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]]) @ np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]])
    return np.concatenate([R, np.asarray(t, dtype=np.float64)[:, None]], 1).ravel().tolist()


def depth_image(kind):
    """(H, W) float64 z of the scene"""
    v, u = np.mgrid[0:H, 0:W]
    if kind == "plane":
        return np.full((H, W), 2.0)
    if kind == "steps":          # four quadrants at different depths: sign changes along x and y as well as z
        return 2.0 + 0.25 * (u > W // 2) + 0.125 * (v > H // 2)
    if kind == "tilt":
        return 1.9 + 0.004 * u + 0.003 * v
    raise ValueError(kind)


def frames(kinds, Hp=51, Wp=73, seed=0, dtype=np.uint8, holes=True):
    """B = len(kinds) pairs: padded disp / occ / conf (B,Hp,Wp) float32 and the images (B,3,H,W).  The padded border holds KEPT pixels at
    z = 1.75 (they would change voxels if they were read); with `holes` the first pair has a block of pixels that fail the confidence test
    or the occlusion test and a block that mixes non-finite, zero and negative disparities."""
    g = np.random.default_rng(seed)
    B = len(kinds)
    oy, ox = (Hp - H) // 2, (Wp - W) // 2
    disp = np.full((B, Hp, Wp), 1.0 / 1.75, F)
    occ, conf = np.ones((B, Hp, Wp), F), np.ones((B, Hp, Wp), F)
    for b, kind in enumerate(kinds):
        disp[b, oy:oy + H, ox:ox + W] = (1.0 / depth_image(kind)).astype(F)
    if holes:
        conf[0, oy + 10:oy + 15, ox + 20:ox + 31] = 0.05
        occ[0, oy + 30:oy + 33, ox + 40:ox + 50] = 0.5           # not > occ_min
        vals = np.array((np.nan, np.inf, -np.inf, 0.0, -3.0), F)
        r, c = np.mgrid[0:5, 0:12]
        disp[0, oy + 18:oy + 23, ox + 28:ox + 40] = vals[(c + 2 * r) % 5]
    img = g.integers(0, 256, (B, 3, H, W)).astype(np.uint8)
    if dtype != np.uint8:
        img = (img.astype(np.float32) + g.uniform(-0.6, 0.6, img.shape).astype(np.float32)).astype(dtype)      # also just outside [0, 255]
    return disp, occ, conf, img


# grids: dims, origin, voxel_size, trunc.  A: awkward dims, wider than the view at its near side.  DYADIC: every centre, the plane and the band
# are dyadic numbers, so that projections land on x.5 and sdf on +-trunc exactly.
GRID_A = dict(dims=(19, 13, 11), origin=(-0.9, -0.6, 1.5), voxel_size=0.1, trunc=0.3)
GRID_DYADIC = dict(dims=(17, 12, 9), origin=(-1.0, -0.625, 1.5), voxel_size=0.125, trunc=0.25)
GRID_ROW = dict(dims=(1, 13, 40), origin=(0.05, -0.6, 1.0), voxel_size=0.05, trunc=0.15)
GRID_LONG = dict(dims=(37, 21, 23), origin=(-0.9, -0.5, 1.45), voxel_size=0.05, trunc=0.2)
