"""Drop-in counterparts of the reference's driver glue around ``S2M2.forward`` (src/s2m2/core/utils/model_utils.py,
image_utils.py) -- SURVEY.md section 8f rows 1-2: same names, arguments and return values, pre/post-processing on the device.

* ``load_model``           model_utils.py:11-48 (model-size table, ``CH{C}NTR{n}.pth`` checkpoint, ``my_load_state_dict``)
* ``image_pad``            image_utils.py:27-71 (HIP kernel ``s2m2_image_pad``)
* ``image_crop``           image_utils.py:73-103 (pure slicing)
* ``run_stereo_matching``  model_utils.py:51-95 (pad -> autocast fp16 forward -> crop -> average confidence)
* ``compute_confidence_score``   model_utils.py:98-101
* ``get_pointcloud``       model_utils.py:111-136 (depth from disparity + open3d's RGBD -> point cloud conversion; HIP kernels ``s2m2_cloud``)
* ``get_mesh``             no counterpart in the reference: ``get_pointcloud``'s arguments -> the surface mesh that connects neighbouring
  pixels of similar disparity (HIP kernels ``s2m2_mesh``; ``s2m2_amd.cloud.mesh``)
* ``filter_speckles``      no counterpart in the reference (its demos leave outlier removal to open3d on the host): ``get_pointcloud``'s
  conventions -> the disparity with the small connected components removed (HIP kernels ``s2m2_segment``; ``s2m2_amd.cloud.segment``)
* ``voxel_down_sample``    no counterpart in the reference (its 3D demos hand the full cloud to open3d on the host): ``get_pointcloud``'s
  arguments -> one point per occupied voxel, the centroid and the mean colour (HIP kernels ``s2m2_voxel``; ``s2m2_amd.cloud.voxelize``)
* ``compute_confidence_scores``  the calibration objective (calibration/base.py:15-36 called 20 x 5 times one pair at a time by
  calibration/cem.py:66-72) for a whole population of rectified pairs at once: one batched forward, or sharded over the ranks of a
  ``torch.distributed`` group
* the calibration glue in front of the forward -- ``parse_xml_calibration``, ``load_calibration_data``, ``euler_to_rotation_matrix``,
  ``create_delta_rotation``, ``apply_delta_rotation``, ``build_camera_matrix``, ``compute_stereo_rectification`` (calib_utils.py),
  ``rectify_images`` (image_utils.py:108-136), ``evaluate_sample`` (calibration/base.py), ``cem_calibration`` (calibration/cem.py) and
  ``rectify_population`` -- lives in ``s2m2_amd.rectify`` (HIP kernel ``s2m2_rectify``) and is re-exported here
* ``evaluate``             no counterpart in the reference (its numbers come from benchmark servers): disparity error statistics against
  ground truth on the device -- lives in ``s2m2_amd.evaluate`` (HIP kernel ``s2m2_disp_eval``) and is re-exported here
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from . import hip
from .evaluate import evaluate  # noqa: F401  (re-export)
from .model import S2M2
from .rectify import (apply_delta_rotation, build_camera_matrix, cem_calibration, compute_stereo_rectification,  # noqa: F401  (re-exports)
                      create_delta_rotation, euler_to_rotation_matrix, evaluate_sample, load_calibration_data, parse_xml_calibration,
                      rectify_images, rectify_population)
from .spec import MODEL_CONFIGS


def load_model(pretrain_path: str, model_type: str, use_positivity: bool = True, refine_iter: int = 3, device=None) -> Optional[S2M2]:
    """Same contract as the reference: returns the model in eval mode on ``device``, or None (after printing) when loading fails."""
    if model_type not in MODEL_CONFIGS:
        print("model type should be one of [S, M, L, XL]")
        raise SystemExit(1)
    c, ntr = MODEL_CONFIGS[model_type]
    ckpt_path = os.path.join(pretrain_path, f"CH{c}NTR{ntr}.pth")
    model = S2M2(feature_channels=c, dim_expansion=1, num_transformer=ntr, use_positivity=use_positivity, refine_iter=refine_iter)
    try:
        checkpoint = torch.load(ckpt_path, weights_only=True)
        model.my_load_state_dict(checkpoint["state_dict"])
        model.eval()
        if device:
            model = model.to(device)
        print("Model loaded")
        return model
    except Exception as e:  # noqa: BLE001  (the reference swallows and reports)
        print(f"Error loading model: {e}")
        return None


def image_pad(img: torch.Tensor, factor: int = 32) -> torch.Tensor:
    """(B,C,H,W) -> (B,C,ceil(H/f)*f,ceil(W/f)*f) fp32 with the reference's blurred border; device tensors only."""
    with torch.cuda.device(img.device):                  # the C ABI launches on the current stream of the current device
        return hip.image_pad(img, factor)


def image_crop(img: torch.Tensor, img_shape: Tuple[int, int]) -> torch.Tensor:
    H, W = img.shape[-2:]
    Hn, Wn = img_shape
    ch = H - Hn
    if ch > 0:
        img = img[:, :, ch // 2: -(ch - ch // 2)]
    cw = W - Wn
    if cw > 0:
        img = img[:, :, :, cw // 2: -(cw - cw // 2)]
    return img


@torch.no_grad()
def run_stereo_matching(model: S2M2, left_torch: torch.Tensor, right_torch: torch.Tensor, device, N_repeat: int = 1):
    """-> (pred_disp, pred_occ, pred_conf, avg_conf_score, run_time_ms); images (1,3,H,W) of any size (padded to x32 here)."""
    img_height, img_width = left_torch.shape[-2:]
    left_pad = image_pad(left_torch.to(device), 32)
    right_pad = image_pad(right_torch.to(device), 32)
    with torch.inference_mode():
        with torch.amp.autocast(enabled=True, device_type=torch.device(device).type, dtype=torch.float16):
            if N_repeat > 1:
                # run-time estimation: the first call with a new geometry runs eagerly and the second captures the hipGraph; keep both
                # out of the timed loop (a single-shot call, N_repeat = 1, is timed as it is)
                # (bounded: with S2M2_GRAPH_CACHE=0, or a batch that forward() slices, no graph for this shape ever becomes resident)
                for _ in range(3):
                    if model.is_warm(left_pad.shape, torch.float16) or os.environ.get("S2M2_GRAPH", "1") == "0":
                        break
                    model(left_pad, right_pad)
            starter, ender = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            starter.record()
            for _ in range(N_repeat):
                pred_disp, pred_occ, pred_conf = model(left_pad, right_pad)
            ender.record()
            torch.cuda.synchronize()
    run_time = starter.elapsed_time(ender) / N_repeat
    pred_disp = image_crop(pred_disp, (img_height, img_width)).squeeze().float()
    pred_occ = image_crop(pred_occ, (img_height, img_width)).squeeze().float()
    pred_conf = image_crop(pred_conf, (img_height, img_width)).squeeze().float()
    margin = 100
    avg_conf_score = pred_conf[margin:-margin, margin:-margin].mean().item()
    return pred_disp, pred_occ, pred_conf, avg_conf_score, run_time


def compute_confidence_score(model: S2M2, left_torch: torch.Tensor, right_torch: torch.Tensor, device) -> float:
    return run_stereo_matching(model, left_torch, right_torch, device, N_repeat=1)[3]


@torch.no_grad()
def compute_confidence_scores(model: S2M2, lefts: torch.Tensor, rights: torch.Tensor, device, batch: Optional[int] = None,
                              dist=None, group=None, margin: int = 100) -> torch.Tensor:
    """Average confidence of N rectified pairs ``lefts`` / ``rights`` (N,3,H,W), same number per pair as ``compute_confidence_score``
    returns for it (pad to x32 -> autocast fp16 forward -> crop -> mean of the confidence map inside a ``margin`` border), evaluated
    ``batch`` pairs per forward (default: all at once; pairs are independent along the batch axis).

    With ``dist`` (an initialised ``torch.distributed`` module, one rank per GPU) the pairs are sharded round-robin over the ranks
    of ``group`` -- every rank passes the full population -- and every rank receives all N scores: the only collective is one
    all-gather of ceil(N/world) floats per rank (N need not divide: short shards are padded and the padding dropped).  Returns a float32 CPU tensor (N,)."""
    N = lefts.shape[0]
    if rights.shape != lefts.shape or lefts.dim() != 4:
        raise ValueError(f"expected two (N,3,H,W) batches, got {tuple(lefts.shape)} and {tuple(rights.shape)}")
    H, W = lefts.shape[-2:]
    if H <= 2 * margin or W <= 2 * margin:
        raise ValueError(f"images of {W}x{H} have no interior inside a {margin}-px margin")
    idx = list(range(N))
    world = rank = 1
    if dist is not None:
        from .shard import padded_shard, shard_indices
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        idx, _ = padded_shard(N, rank, world)                # N % world != 0: pad and drop, the all-gather stays fixed-size
    step = batch or max(1, len(idx))
    scores = []
    for s0 in range(0, len(idx), step):
        sel = idx[s0:s0 + step]
        lp = image_pad(lefts[sel].to(device), 32)
        rp = image_pad(rights[sel].to(device), 32)
        with torch.amp.autocast(enabled=True, device_type=torch.device(device).type, dtype=torch.float16):
            conf = model(lp, rp)[2]
        conf = image_crop(conf, (H, W)).float()
        scores.append(conf[:, 0, margin:-margin, margin:-margin].mean(dim=(1, 2)))
    mine = torch.cat(scores) if scores else torch.empty(0, device=device)
    if dist is None:
        return mine.cpu()
    parts = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(parts, mine, group=group)
    out = torch.empty(N, dtype=torch.float32)
    for r in range(world):
        real = shard_indices(N, r, world)
        out[real] = parts[r][:len(real)].float().cpu()
    return out


def get_pointcloud(rgb, disp, calib, depth_trunc=None):
    """Same arguments as the reference: ``rgb`` (H,W,3) uint8, ``disp`` (H,W) (numpy arrays or tensors), ``calib`` the dict of
    ``cloud.read_calib_file`` -- including the reference's halving of fx, cx and cy (it is written for half-resolution Middlebury images) and
    fx for both focal lengths.  No confidence filter, like the reference function: the caller passes the disparity already filtered (-1 where
    invalid).  Returns a ``cloud.PointCloud`` on the device instead of an open3d object."""
    from . import cloud
    disp_t = torch.as_tensor(disp)
    device = disp_t.device if disp_t.is_cuda else torch.device("cuda")
    disp_t = disp_t.to(device=device, dtype=torch.float32).contiguous()[None, None]
    image = torch.as_tensor(rgb).to(device).permute(2, 0, 1).contiguous()[None]
    cam0 = calib["cam0"]
    with torch.cuda.device(device):
        return cloud.reproject(disp_t, disp_t, disp_t, image, fx=float(cam0[0, 0]) / 2.0, cx=float(cam0[0, 2]) / 2.0, cy=float(cam0[1, 2]) / 2.0,
                               baseline=float(calib["baseline"]), doffs=float(calib["doffs"]), depth_trunc=depth_trunc, filtered=False)


def get_mesh(rgb, disp, calib, depth_trunc=None, max_jump=1.0):
    """``get_pointcloud``'s arguments and conventions (halved intrinsics, fx for both focal lengths, no confidence filter) -> a ``cloud.Mesh`` on
    the device: the same vertices plus the triangles between neighbouring pixels whose disparities differ by at most ``max_jump`` px."""
    from . import cloud
    disp_t = torch.as_tensor(disp)
    device = disp_t.device if disp_t.is_cuda else torch.device("cuda")
    disp_t = disp_t.to(device=device, dtype=torch.float32).contiguous()[None, None]
    image = torch.as_tensor(rgb).to(device).permute(2, 0, 1).contiguous()[None]
    cam0 = calib["cam0"]
    with torch.cuda.device(device):
        return cloud.mesh(disp_t, disp_t, disp_t, image, fx=float(cam0[0, 0]) / 2.0, cx=float(cam0[0, 2]) / 2.0, cy=float(cam0[1, 2]) / 2.0,
                          baseline=float(calib["baseline"]), doffs=float(calib["doffs"]), depth_trunc=depth_trunc, filtered=False,
                          max_jump=max_jump)


def get_normals(disp, calib, depth_trunc=None, radius=1, max_jump=1.0, min_cos=0.0):
    """``get_pointcloud``'s conventions (halved intrinsics, fx for both focal lengths, no confidence filter: ``disp`` (H,W) arrives filtered, -1
    where invalid) -> a ``cloud.NormalMap`` on the device: the depth map and the unit normal of every kept pixel in the camera frame, from the
    neighbours ``radius`` pixels away whose disparities differ by at most ``max_jump * radius`` px, kept where the cosine with the direction to
    the camera is at least ``min_cos``.  ``PointCloud.write_ply(..., normals=...)`` and ``Mesh.write_ply`` take it."""
    from . import cloud
    disp_t = torch.as_tensor(disp)
    device = disp_t.device if disp_t.is_cuda else torch.device("cuda")
    disp_t = disp_t.to(device=device, dtype=torch.float32).contiguous()[None, None]
    cam0 = calib["cam0"]
    with torch.cuda.device(device):
        return cloud.normals(disp_t, disp_t, disp_t, fx=float(cam0[0, 0]) / 2.0, cx=float(cam0[0, 2]) / 2.0, cy=float(cam0[1, 2]) / 2.0,
                             baseline=float(calib["baseline"]), doffs=float(calib["doffs"]), depth_trunc=depth_trunc, filtered=False,
                             radius=radius, max_jump=max_jump, min_cos=min_cos)


def smooth_disparity(disp, calib, sigma_r, max_jump, depth_trunc=None, radius=2, sigma_s=None):
    """``get_normals``'s conventions (halved intrinsics, fx for both focal lengths, no confidence filter: ``disp`` (H,W) arrives filtered, -1
    where invalid) -> a ``cloud.Smoothed`` on the device: the disparity map after the edge-preserving filter of ``cloud.smooth`` (a window of
    (2 ``radius`` + 1)^2 pixels, the widths ``sigma_s`` pixels -- None: ``radius / 2`` -- and ``sigma_r`` px of disparity, neighbours within
    ``max_jump`` px of the centre), -1 where the pixel is not kept.  ``.disp[0, 0]`` stands wherever ``disp`` stood."""
    from . import cloud
    disp_t = torch.as_tensor(disp)
    device = disp_t.device if disp_t.is_cuda else torch.device("cuda")
    disp_t = disp_t.to(device=device, dtype=torch.float32).contiguous()[None, None]
    cam0 = calib["cam0"]
    with torch.cuda.device(device):
        return cloud.smooth(disp_t, disp_t, disp_t, fx=float(cam0[0, 0]) / 2.0, cx=float(cam0[0, 2]) / 2.0, cy=float(cam0[1, 2]) / 2.0,
                            baseline=float(calib["baseline"]), doffs=float(calib["doffs"]), depth_trunc=depth_trunc, filtered=False,
                            radius=radius, sigma_s=sigma_s, sigma_r=sigma_r, max_jump=max_jump)


def voxel_down_sample(rgb, disp, calib, voxel_size, depth_trunc=None):
    """``get_pointcloud``'s arguments and conventions (halved intrinsics, fx for both focal lengths, no confidence filter) -> a
    ``cloud.VoxelCloud`` on the device: one point per occupied cell of a grid of ``voxel_size`` (the unit of z: metres with a Middlebury
    calibration) anchored at the camera, the centroid and the mean colour of the cell's points, with the number of points per cell."""
    from . import cloud
    disp_t = torch.as_tensor(disp)
    device = disp_t.device if disp_t.is_cuda else torch.device("cuda")
    disp_t = disp_t.to(device=device, dtype=torch.float32).contiguous()[None, None]
    image = torch.as_tensor(rgb).to(device).permute(2, 0, 1).contiguous()[None]
    cam0 = calib["cam0"]
    with torch.cuda.device(device):
        return cloud.voxelize(disp_t, disp_t, disp_t, image, fx=float(cam0[0, 0]) / 2.0, cx=float(cam0[0, 2]) / 2.0, cy=float(cam0[1, 2]) / 2.0,
                              baseline=float(calib["baseline"]), doffs=float(calib["doffs"]), depth_trunc=depth_trunc, filtered=False,
                              voxel_size=voxel_size)


def integrate_tsdf(volume, rgb, disp, calib, R, t, depth_trunc=None):
    """``get_pointcloud``'s arguments and conventions (halved intrinsics, fx for both focal lengths, no confidence filter) for one frame of a
    moving rig: the frame's depth map is fused into ``volume`` (a ``cloud.TsdfVolume``) from the pose ``R`` (3,3), ``t`` (3,) -- world ->
    camera, ``t`` in the unit of z (metres with a Middlebury calibration).  Returns ``volume``."""
    disp_t = torch.as_tensor(disp).to(device=volume.device, dtype=torch.float32).contiguous()[None, None]
    image = torch.as_tensor(rgb).to(volume.device).permute(2, 0, 1).contiguous()[None]
    cam0 = calib["cam0"]
    with torch.cuda.device(volume.device):
        volume.integrate(disp_t, disp_t, disp_t, image, R=R, t=t, fx=float(cam0[0, 0]) / 2.0, cx=float(cam0[0, 2]) / 2.0,
                         cy=float(cam0[1, 2]) / 2.0, baseline=float(calib["baseline"]), doffs=float(calib["doffs"]), depth_trunc=depth_trunc,
                         filtered=False)
    return volume


def render_tsdf(volume, calib, R, t, size=None):
    """``get_pointcloud``'s conventions (halved intrinsics, fx for both focal lengths) -> ``volume`` (a ``cloud.TsdfVolume``) seen from the pose
    ``R`` (3,3), ``t`` (3,), world -> camera as ``integrate_tsdf`` takes it: a ``cloud.TsdfRender`` on the device with the model's depth,
    normals and colour.  ``size`` = (width, height) of the rendered maps; None: half the calibration's ``width`` and ``height``."""
    from . import cloud
    cam0 = calib["cam0"]
    if size is None:
        size = (int(calib["width"]) // 2, int(calib["height"]) // 2)
    camera = cloud.Camera(size[0], size[1], float(cam0[0, 0]) / 2.0, float(cam0[0, 0]) / 2.0, float(cam0[0, 2]) / 2.0, float(cam0[1, 2]) / 2.0)
    with torch.cuda.device(volume.device):
        return volume.raycast(camera, R, t)


def track_tsdf(volume, disp, calib, R, t, depth_trunc=None, n_iters=10, **gates):
    """``integrate_tsdf``'s conventions (halved intrinsics, fx for both focal lengths, no confidence filter) for the pose of a new frame:
    ``volume`` (a ``cloud.TsdfVolume``) is rendered from the guess ``R`` (3,3), ``t`` (3,) at the size of ``disp`` (H,W), and the frame is
    tracked against that render from the same guess (``cloud.TsdfVolume.track``; ``gates``: its max_dist, min_count, max_rot, max_trans).
    Returns ``(R, t, ok)``: (3,3) and (3,) fp32 tensors on the device, as the accepted iterations left them, and whether the last
    iteration was accepted (read on the host: synchronises)."""
    disp_t = torch.as_tensor(disp).to(device=volume.device, dtype=torch.float32).contiguous()[None, None]
    H, W = disp_t.shape[-2:]
    cam0 = calib["cam0"]
    with torch.cuda.device(volume.device):
        render = render_tsdf(volume, calib, R, t, size=(W, H))
        tr = volume.track(disp_t, disp_t, disp_t, render, R=R, t=t, fx=float(cam0[0, 0]) / 2.0, cx=float(cam0[0, 2]) / 2.0,
                          cy=float(cam0[1, 2]) / 2.0, baseline=float(calib["baseline"]), doffs=float(calib["doffs"]), depth_trunc=depth_trunc,
                          filtered=False, n_iters=n_iters, **gates)
    return tr.R[0], tr.t[0], tr.ok(0)


def filter_speckles(disp, calib, depth_trunc=None, max_jump=1.0, min_size=100):
    """``get_pointcloud``'s conventions (halved intrinsics, fx for both focal lengths, no confidence filter: ``disp`` (H,W) arrives filtered, -1
    where invalid) -> the (H,W) fp32 disparity on the device with -1 also wherever the pixel's 4-connected component of similar disparity
    (neighbours differ by at most ``max_jump`` px) has fewer than ``min_size`` pixels: the speckle filter in front of ``get_pointcloud`` /
    ``get_mesh``."""
    from . import cloud
    disp_t = torch.as_tensor(disp)
    device = disp_t.device if disp_t.is_cuda else torch.device("cuda")
    disp_t = disp_t.to(device=device, dtype=torch.float32).contiguous()[None, None]
    H, W = disp_t.shape[-2:]
    cam0 = calib["cam0"]
    with torch.cuda.device(device):
        s = cloud.segment(disp_t, disp_t, disp_t, H=H, W=W, fx=float(cam0[0, 0]) / 2.0, cx=float(cam0[0, 2]) / 2.0, cy=float(cam0[1, 2]) / 2.0,
                          baseline=float(calib["baseline"]), doffs=float(calib["doffs"]), depth_trunc=depth_trunc, filtered=False,
                          max_jump=max_jump, min_size=min_size, want_label=False, want_size=False)
    return s.disp[0, 0]
