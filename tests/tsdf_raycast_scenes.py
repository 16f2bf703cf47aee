"""Scenes shared by the CPU and GPU tests of K26: target cameras, poses, volumes written straight into the buffer and the dyadic "ties" scene.
Nothing here computes an expected result: that is tsdf_raycast_oracle's."""
import numpy as np

import tsdf_oracle as O
import tsdf_scenes as S

F = np.float32

# a target camera whose numbers are no powers of two, 37 rows x 53 columns, and the scenes' own 45 x 67
CAM_ODD = dict(Ht=37, Wt=53, fx=41.3, fy=39.7, cx=25.9, cy=17.3)
CAM_OWN = dict(Ht=S.H, Wt=S.W, fx=S.CAM["fx"], fy=S.CAM["fy"], cx=S.CAM["cx"], cy=S.CAM["cy"])

ROT = S.rot_xy(0.1, -0.15, (0.05, -0.03, 0.1))
AWAY = [-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0]            # half a turn about y: the camera looks along -z, away from every grid of tsdf_scenes
POSES3 = np.array([S.IDENTITY, ROT, AWAY], F)


def place(grid):
    return dict(origin=grid["origin"], voxel_size=grid["voxel_size"])


def march(grid, z_near=0.0, z_far=4.0, step=None):
    """the range and the step of a render of `grid`: every grid of tsdf_scenes ends in front of z = 4"""
    return dict(z_near=z_near, z_far=z_far, step=grid["trunc"] / 2 if step is None else step)


def fuse(grid, kinds=("plane", "steps", "tilt"), poses=None, max_weight=64, seed=0):
    """tsdf_scenes' frames fused by tsdf_oracle (what test_hip_tsdf_mesh._fuse does)"""
    poses = np.array([S.IDENTITY, ROT, S.IDENTITY], F)[:len(kinds)] if poses is None else np.asarray(poses, F)
    vol, _ = O.integrate(O.empty(grid["dims"]), *S.frames(list(kinds), seed=seed), poses, **place(grid), trunc=grid["trunc"], max_weight=max_weight,
                         **S.CAM)
    return vol


RANDOM_GRID = dict(dims=(20, 19, 18), origin=(-0.45, -0.5, 1.25), voxel_size=0.05, trunc=0.2)


def random_volume(dims, seed, unobserved=0.0):
    """random signs and magnitudes written straight into the buffer, colours that differ from voxel to voxel"""
    g = np.random.default_rng(seed)
    Nx, Ny, Nz = dims
    vol = O.empty(dims)
    vol[..., 0] = g.uniform(-1, 1, (Nz, Ny, Nx)).astype(F).view(np.int32)
    vol[..., 1] = np.where(g.random((Nz, Ny, Nx)) < unobserved, 0, g.integers(1, 5, (Nz, Ny, Nx)))
    vol[..., 2] = g.integers(0, 65281, (Nz, Ny, Nx)) | g.integers(0, 65281, (Nz, Ny, Nx)) << 16
    vol[..., 3] = g.integers(0, 65281, (Nz, Ny, Nx))
    return vol


# ---- ties: every number a dyadic one.  Voxels of 1/8 from x = -1/2, y = -1/2, z = 1; a 9 x 9 camera with fx = fy = 64 whose central ray
# (u = v = 4) runs along +z through the voxel centres of one column: with the camera moved by whole voxels in x (TIES_POSES) through the columns
# i = 4, 6 and 8, j = 4.  With z_near = 0 and step = 1/8 the samples of a central ray are voxel centres (fr == 0 on all axes) and sample 16 lies
# on g_z == Nz - 1; with z_near = 1/16 they lie half way between two centres (fr_z == 0.5).
TIES_GRID = dict(dims=(11, 9, 9), origin=(-0.5, -0.5, 1.0), voxel_size=0.125, trunc=0.25)
TIES_CAM = dict(Ht=9, Wt=9, fx=64.0, fy=64.0, cx=4.0, cy=4.0)
TIES_POSES = np.array([[1, 0, 0, -0.125 * m, 0, 1, 0, 0, 0, 0, 1, 0] for m in (0, 2, 4)], F)


def ties_volume():
    """column (4, 4): positive throughout (its central ray reaches g_z == Nz - 1); column (6, 4): 1, 0.5, +0.0, -0.5, ... (a crossing behind an
    exact zero: z_hit is the zero's sample); column (8, 4): 1, -0.0, -0.0, -1, ... with smaller values all around, so that the interpolation
    keeps the sign of the zero.  Everywhere else a plane near z = 1.4 tilted in x and y; colours differ from voxel to voxel."""
    Nx, Ny, Nz = TIES_GRID["dims"]
    k, j, i = np.mgrid[0:Nz, 0:Ny, 0:Nx]
    t = (F(0.4) - k.astype(F) * F(0.125)) + (i - 5).astype(F) * F(0.03125) + (j - 4).astype(F) * F(0.015625)
    t = t.astype(F)
    t[:, 4, 4] = 0.75
    t[:, 4, 6] = np.array([1, 0.5, 0.0, -0.5, -1, -1, -1, -1, -1], F)
    t[:, 3:6, 7:10] = np.array([0.5, -0.25, -0.25, -1, -1, -1, -1, -1, -1], F)[:, None, None]
    t[:, 4, 8] = np.array([1, -0.0, -0.0, -1, -1, -1, -1, -1, -1], F)
    vol = O.empty(TIES_GRID["dims"])
    vol[..., 0] = t.view(np.int32)
    vol[..., 1] = 1
    lin = np.arange(t.size, dtype=np.int64).reshape(t.shape)
    vol[..., 2] = ((lin * 37) % 65281 | ((lin * 101) % 65281) << 16).astype(np.int32)
    vol[..., 3] = ((lin * 53) % 65281).astype(np.int32)
    return vol
