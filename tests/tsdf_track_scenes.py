"""Scenes shared by the CPU and GPU tests of K27.  The plane, steps and tilt scenes of tsdf_scenes cannot constrain six degrees of freedom, so
the tracking scene is a curved surface: fused by tsdf_oracle at the identity, the model maps rendered by tsdf_raycast_oracle, and the live frame
rendered by the same oracle from the TRUE pose (disparity = 1 / z, holes as disparity 0).  Nothing here computes an expected tracking result:
that is tsdf_track_oracle's.  Everything is computed once per process."""
import functools

import numpy as np

import tsdf_oracle as O
import tsdf_raycast_oracle as RO
import tsdf_raycast_scenes as RS
import tsdf_scenes as S

F = np.float32
GRID = S.GRID_LONG
TRUE = S.rot_xy(0.02, -0.03, (0.02, -0.01, 0.03))          # the live camera of the tracking scene, world -> camera
PARTIAL = S.rot_xy(0.02, 0.05, (0.27, -0.01, 0.05))        # a start from which only a part of the live frame meets the model image
LOST = S.rot_xy(0.0, 0.3, (0.55, 0.0, 0.1))                # ... and one whose first step is longer than GATES allow (status 3)
CAM_LIVE = {k: S.CAM[k] for k in ("fx", "fy", "cx", "cy", "baseline", "doffs", "depth_scale", "depth_trunc", "conf_min", "occ_min")}
CAM_BIG = dict(CAM_LIVE, fx=128.0, fy=128.0, cx=67.0, cy=45.0, depth_scale=128.0)       # 92 x 134: four tiles of thirty rows, the last of two; W % 4 == 2
GATES = dict(max_dist=GRID["trunc"], min_count=6, max_rot=0.5, max_trans=0.5)


def curved_depth(H=S.H, W=S.W):
    v, u = np.mgrid[0:H, 0:W]
    return 2.0 + 0.12 * np.sin(u / 7.0) + 0.10 * np.cos(v / 5.0) + 0.08 * np.sin((u + v) / 9.0)


def pad(depth, Hp, Wp, border=1.75, scale=1.0):
    """(H,W) depth with 0 = hole -> padded disp / occ / conf (Hp,Wp): disparity = scale / z, holes as disparity 0; the padded border holds KEPT
    pixels at z = `border` (they would change the sums if they were read)"""
    H, W = depth.shape
    oy, ox = (Hp - H) // 2, (Wp - W) // 2
    disp = np.full((Hp, Wp), scale / border, F)
    with np.errstate(divide="ignore"):
        disp[oy:oy + H, ox:ox + W] = np.where(depth > 0, F(scale) / depth.astype(F), F(0))
    return disp, np.ones((Hp, Wp), F), np.ones((Hp, Wp), F)


@functools.lru_cache(None)
def volume():
    """the curved surface fused at the identity into GRID_LONG with carve"""
    disp, occ, conf = pad(curved_depth(), 51, 73)
    img = np.random.default_rng(5).integers(0, 256, (1, 3, S.H, S.W)).astype(np.uint8)
    vol, _ = O.integrate(O.empty(GRID["dims"]), disp[None], occ[None], conf[None], img, np.array([S.IDENTITY], F), **RS.place(GRID),
                         trunc=GRID["trunc"], max_weight=64, carve=True, **S.CAM)
    return vol


@functools.lru_cache(None)
def render(pose=tuple(S.IDENTITY), cam="own"):
    """depth (Ht,Wt) and gradients (3,Ht,Wt) of volume() from `pose` through CAM_OWN, CAM_ODD, the 92 x 134 camera, or the row / column through the principal point"""
    camera = dict(own=RS.CAM_OWN, odd=RS.CAM_ODD, big=dict(Ht=92, Wt=134, fx=128.0, fy=128.0, cx=67.0, cy=45.0),
                  row=dict(RS.CAM_OWN, Ht=1, cy=0.0), col=dict(RS.CAM_OWN, Wt=1, cx=0.0))[cam]
    r = RO.raycast(volume(), np.array([pose], F), **camera, **RS.place(GRID), **RS.march(GRID))
    return r["depth"][0, 0], r["gradients"][0], camera


def model_kw(cam="own"):
    c = render(cam=cam)[2]
    return dict(mfx=c["fx"], mfy=c["fy"], mcx=c["cx"], mcy=c["cy"])


@functools.lru_cache(None)
def live(cam="own", Hp=51, Wp=73, pose=tuple(TRUE)):
    """the padded live maps (Hp,Wp) of the frame seen from `pose`, and its H, W and camera keywords"""
    depth, _, c = render(pose, cam)
    kw = dict(CAM_BIG if cam == "big" else CAM_LIVE, cx=c["cx"], cy=c["cy"], H=c["Ht"], W=c["Wt"])
    return pad(depth, Hp, Wp), kw


def spoiled_model():
    """render() with blocks of zero, NaN and Inf gradients and of NaN, negative and Inf depths: none of them may become a correspondence"""
    md, mg, _ = render()
    md, mg = md.copy(), mg.copy()
    mg[:, 10:14, 20:26] = 0.0
    mg[0, 16:18, 20:26] = np.nan
    mg[1, 20:22, 20:26] = np.inf
    md[24:26, 20:26] = np.nan
    md[28:30, 20:26] = -1.0
    md[32:34, 20:26] = np.inf
    return md, mg


@functools.lru_cache(None)
def plane_model():
    """the dyadic plane z = 2 fused at the identity into GRID_DYADIC and rendered from the identity through a camera of powers of two: the
    gradients are (0, 0, g) exactly"""
    vol = RS.fuse(S.GRID_DYADIC, kinds=("plane",), poses=[S.IDENTITY])
    cam = dict(Ht=S.H, Wt=S.W, fx=64.0, fy=64.0, cx=33.5, cy=22.5)
    r = RO.raycast(vol, np.array([S.IDENTITY], F), **cam, **RS.place(S.GRID_DYADIC), **RS.march(S.GRID_DYADIC))
    return r["depth"][0, 0], r["gradients"][0]


def plane_live(Hp=51, Wp=73):
    return pad(np.full((S.H, S.W), 2.0), Hp, Wp)
