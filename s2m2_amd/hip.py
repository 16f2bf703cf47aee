"""ctypes binding of libs2m2_hip.so (include/s2m2_hip.h) for PyTorch-ROCm tensors.

PyTorch is plumbing here: it owns device memory and the stream; every function below enqueues hand-written
gfx950 kernels on ``torch.cuda.current_stream()`` through the C ABI.  There is NO fallback: if the shared
library is missing or a call fails, a RuntimeError is raised.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from typing import Optional, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libs2m2_hip%s.so" % os.environ.get("S2M2_LIB_SUFFIX", ""))   # suffix: experiment builds only

F32, F16 = 0, 1
_DT = {torch.float32: F32, torch.float16: F16}

_lib: Optional[ctypes.CDLL] = None

_vp, _i, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong

ACT_NONE, ACT_GELU, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3, 4
EPI_NONE, EPI_ADD, EPI_MUL, EPI_GRU, EPI_GATEMIX, EPI_DUALMIX = 0, 1, 2, 3, 4, 5


class ConvDesc(ctypes.Structure):
    """mirror of s2m2_conv_desc (include/s2m2_hip.h)"""
    _fields_ = [("src", _vp * 4), ("src_c", _i * 4), ("src_stride", _i * 4), ("nsrc", _i), ("weight", _vp), ("bias", _vp),
                ("out", _vp), ("out_stride", _i), ("N", _i), ("H", _i), ("W", _i), ("KH", _i), ("KW", _i), ("Cout", _i),
                ("act", _i), ("epi", _i), ("aux0", _vp), ("aux1", _vp), ("aux0_stride", _i), ("aux1_stride", _i),
                ("out_scale", ctypes.c_float), ("shuffle2", _i), ("tile", _i), ("dtype", _i), ("korder", _i), ("stride", _i),
                ("ln_wsum", _vp), ("ln_eps", ctypes.c_float), ("ksplit", _i), ("bias2", _vp), ("pool2", _i), ("epi_cout0", _i)]


class ChainDesc(ctypes.Structure):
    """mirror of s2m2_chain_desc (include/s2m2_hip.h)"""
    _fields_ = [("x", _vp), ("res", _vp), ("out", _vp), ("x_stride", _ll), ("res_stride", _ll), ("out_stride", _ll), ("rows", _ll),
                ("C", _i), ("nstage", _i), ("weight", _vp * 3), ("bias", _vp * 3), ("ln_wsum", _vp * 3), ("act", _i * 3),
                ("res_stage", _i), ("carry", _i), ("ln_eps", ctypes.c_float), ("dtype", _i),
                ("ln_out", _vp), ("ln_out_stride", _ll), ("ln_gamma", _vp), ("ln_beta", _vp), ("ln_out_eps", ctypes.c_float),
                ("fan_weight", _vp), ("fan_bias", _vp), ("fan_ln_wsum", _vp), ("fan_out", _vp), ("fan_out_stride", _ll),
                ("nfan", _i), ("xcd_group_rows", _ll), ("weight_frag", _i), ("pool_h", _i), ("pool_w", _i)]


class RowAttnDesc(ctypes.Structure):
    """mirror of s2m2_rowattn_desc (include/s2m2_hip.h): K13, one 1-D attention step per launch"""
    _fields_ = [("x", _vp), ("x_stride", _ll), ("out", _vp), ("out_stride", _ll), ("nimg", _i), ("h", _i), ("w", _i), ("C", _i), ("heads", _i),
                ("cross", _i), ("weights", _vp), ("vectors", _vp), ("ln_eps", ctypes.c_float),
                ("ln_out", _vp), ("ln_out_stride", _ll), ("ln_out_eps", ctypes.c_float), ("xcd_hint", _i), ("dtype", _i)]


class ConvBlockDesc(ctypes.Structure):
    """mirror of s2m2_convblock_desc (include/s2m2_hip.h): K14, a whole ConvBlock2D per launch"""
    _fields_ = [("x", _vp), ("x_stride", _ll), ("out", _vp), ("out_stride", _ll), ("N", _i), ("H", _i), ("W", _i), ("C", _i),
                ("w_conv0", _vp), ("w_conv2", _vp), ("w_1x0", _vp), ("w_1x2", _vp), ("b_conv0", _vp), ("b_conv2", _vp), ("b_1x0", _vp),
                ("b_1x2", _vp), ("patch_rows", _i), ("dtype", _i)]


class ConvGruDesc(ctypes.Structure):
    """mirror of s2m2_convgru_desc (include/s2m2_hip.h): K17, one ConvGRU half per launch"""
    _fields_ = [("h", _vp), ("h_stride", _ll), ("x", _vp), ("x_stride", _ll), ("out", _vp), ("out_stride", _ll), ("N", _i), ("H", _i), ("W", _i),
                ("C", _i), ("KH", _i), ("KW", _i), ("w_zr", _vp), ("w_q", _vp), ("b_zr", _vp), ("b_q", _vp), ("dtype", _i)]


class ConvTailDesc(ctypes.Structure):
    """mirror of s2m2_convtail_desc (include/s2m2_hip.h): K19, the second half of a ConvBlock2D per launch"""
    _fields_ = [("t", _vp), ("t_stride", _ll), ("z", _vp), ("z_stride", _ll), ("out", _vp), ("out_stride", _ll), ("N", _i), ("H", _i), ("W", _i),
                ("C", _i), ("w_conv2", _vp), ("w_1x0", _vp), ("w_1x2", _vp), ("b_conv2", _vp), ("b_1x0", _vp), ("b_1x2", _vp), ("patch_rows", _i),
                ("patch_cols", _i), ("dtype", _i)]


class PwDesc(ctypes.Structure):
    """mirror of s2m2_pw_desc (include/s2m2_hip.h)"""
    _fields_ = [("src", _vp * 4), ("src_c", _i * 4), ("src_stride", _ll * 4), ("nsrc", _i), ("rows", _ll), ("weight_frag", _vp), ("bias", _vp),
                ("out", _vp), ("out_stride", _ll), ("Cout", _i), ("act", _i), ("shuffle2", _i), ("Ho", _i), ("Wo", _i), ("dtype", _i)]


class NarrowDesc(ctypes.Structure):
    """mirror of s2m2_narrow_desc (include/s2m2_hip.h)"""
    _fields_ = [("x", _vp), ("x_stride", _ll), ("N", _i), ("H", _i), ("W", _i), ("Cin", _i), ("x1", _vp), ("x1_stride", _ll), ("Cin1", _i),
                ("weight_frag", _vp), ("bias", _vp), ("out", _vp), ("out_stride", _ll), ("Cout", _i), ("KH", _i), ("KW", _i), ("stride", _i),
                ("act", _i), ("dtype", _i), ("head_frag", _vp), ("head_bias", _vp), ("head_cout", _i)]


class CorrDesc(ctypes.Structure):
    """mirror of s2m2_corr_desc (include/s2m2_hip.h): every form of K1"""
    _fields_ = [("tokens", _vp), ("ln_weight", _vp), ("ln_bias", _vp), ("cv", _vp), ("B", _i), ("h", _i), ("w", _i), ("C", _i),
                ("cv_pitch", _i), ("band", _i), ("token_dtype", _i), ("cv_dtype", _i), ("start_event", _vp), ("stop_event", _vp)]


class PackDesc(ctypes.Structure):
    """mirror of s2m2_pack_desc (include/s2m2_hip.h): weight packing into the fragment orders of the direct-form kernels"""
    _fields_ = [("kind", _i), ("w", _vp), ("w2", _vp), ("rows", _i), ("cols", _i), ("ld", _i), ("ld2", _i), ("ntap", _i), ("out", _vp),
                ("out_elems", _ll)]


PACK_ROWS, PACK_NARROW, PACK_CONV_FRAG, PACK_FUSION, PACK_HEAD = range(5)

REGION_CONTENT, REGION_SCRATCH, REGION_EXTERNAL = range(3)


class EngineRegion(ctypes.Structure):
    """mirror of s2m2_engine_region (include/s2m2_hip.h)"""
    _fields_ = [("base", _vp), ("bytes", ctypes.c_ulonglong), ("kind", _i)]


class EngineInfo(ctypes.Structure):
    """mirror of s2m2_engine_info (include/s2m2_hip.h)"""
    _fields_ = [("B", _i), ("H", _i), ("W", _i), ("dtype", _i), ("image_dtype", _i), ("feature_channels", _i), ("dim_expansion", _i),
                ("num_transformer", _i), ("use_positivity", _i), ("output_upsample", _i), ("refine_iter", _i), ("out_h", _i), ("out_w", _i),
                ("out_region", _i), ("out_offset", _ll)]


class CloudDesc(ctypes.Structure):
    """mirror of s2m2_cloud_desc (include/s2m2_hip.h): K15, the 3D output stage"""
    _fields_ = [("disp", _vp), ("occ", _vp), ("conf", _vp), ("image", _vp), ("depth", _vp), ("mask", _vp), ("records", _vp), ("count", _vp),
                ("workspace", _vp), ("B", _i), ("H", _i), ("W", _i), ("Hp", _i), ("Wp", _i), ("image_dtype", _i), ("unfiltered", _i),
                ("capacity", _ll), ("fx", ctypes.c_double), ("fy", ctypes.c_double), ("cx", ctypes.c_double), ("cy", ctypes.c_double),
                ("baseline", ctypes.c_double), ("doffs", ctypes.c_double), ("depth_scale", ctypes.c_double), ("depth_trunc", ctypes.c_double),
                ("conf_min", ctypes.c_double), ("occ_min", ctypes.c_double)]


class MeshDesc(ctypes.Structure):
    """mirror of s2m2_mesh_desc (include/s2m2_hip.h): K20, the surface mesh behind the 3D stage"""
    _fields_ = [("cloud", CloudDesc), ("faces", _vp), ("face_count", _vp), ("index", _vp), ("face_capacity", _ll), ("max_jump", ctypes.c_double)]


class RegisterDesc(ctypes.Structure):
    """mirror of s2m2_register_desc (include/s2m2_hip.h): K21, the depth map registered to a second camera"""
    _fields_ = [("cloud", CloudDesc), ("Ht", _i), ("Wt", _i), ("splat", _i), ("fx_t", ctypes.c_double), ("fy_t", ctypes.c_double),
                ("cx_t", ctypes.c_double), ("cy_t", ctypes.c_double), ("R", ctypes.c_double * 9), ("t", ctypes.c_double * 3), ("depth_t", _vp),
                ("index_t", _vp), ("image_t", _vp), ("visible", _vp), ("count", _vp), ("workspace", _vp)]


class SegmentDesc(ctypes.Structure):
    """mirror of s2m2_segment_desc (include/s2m2_hip.h): K22, connected components and the speckle filter"""
    _fields_ = [("cloud", CloudDesc), ("label", _vp), ("size", _vp), ("mask", _vp), ("disp_out", _vp), ("stats", _vp), ("workspace", _vp),
                ("max_jump", ctypes.c_double), ("min_size", _ll)]


class VoxelDesc(ctypes.Structure):
    """mirror of s2m2_voxel_desc (include/s2m2_hip.h): K23, voxel-grid downsampling of the point cloud"""
    _fields_ = [("cloud", CloudDesc), ("records", _vp), ("weights", _vp), ("count", _vp), ("index", _vp), ("stats", _vp), ("workspace", _vp),
                ("voxel_size", ctypes.c_double), ("max_voxels", _ll), ("capacity", _ll)]


class TsdfDesc(ctypes.Structure):
    """mirror of s2m2_tsdf_desc (include/s2m2_hip.h): K24, depth maps fused into a TSDF volume"""
    _fields_ = [("cloud", CloudDesc), ("volume", _vp), ("poses", _vp), ("Nx", _i), ("Ny", _i), ("Nz", _i), ("max_weight", _i), ("carve", _i),
                ("origin", ctypes.c_double * 3), ("voxel_size", ctypes.c_double), ("trunc", ctypes.c_double)]


class TsdfExtractDesc(ctypes.Structure):
    """mirror of s2m2_tsdf_extract_desc (include/s2m2_hip.h): K24, the surface points of a TSDF volume"""
    _fields_ = [("volume", _vp), ("records", _vp), ("gradients", _vp), ("count", _vp), ("workspace", _vp), ("Nx", _i), ("Ny", _i), ("Nz", _i),
                ("min_weight", _i), ("capacity", _ll), ("origin", ctypes.c_double * 3), ("voxel_size", ctypes.c_double)]


class TsdfMeshDesc(ctypes.Structure):
    """mirror of s2m2_tsdf_mesh_desc (include/s2m2_hip.h): K25, the surface of a TSDF volume as a triangle mesh"""
    _fields_ = [("extract", TsdfExtractDesc), ("faces", _vp), ("face_count", _vp), ("face_capacity", _ll)]


class TsdfRaycastDesc(ctypes.Structure):
    """mirror of s2m2_tsdf_raycast_desc (include/s2m2_hip.h): K26, a TSDF volume ray-cast into depth, gradient and colour maps"""
    _fields_ = [("volume", _vp), ("poses", _vp), ("depth", _vp), ("gradients", _vp), ("image", _vp), ("count", _vp), ("B", _i), ("Ht", _i),
                ("Wt", _i), ("Nx", _i), ("Ny", _i), ("Nz", _i), ("min_weight", _i), ("fx", ctypes.c_double), ("fy", ctypes.c_double),
                ("cx", ctypes.c_double), ("cy", ctypes.c_double), ("origin", ctypes.c_double * 3), ("voxel_size", ctypes.c_double),
                ("z_near", ctypes.c_double), ("z_far", ctypes.c_double), ("step", ctypes.c_double)]


class TsdfTrackDesc(ctypes.Structure):
    """mirror of s2m2_tsdf_track_desc (include/s2m2_hip.h): K27, the camera tracked against a TSDF volume's rendered model maps"""
    _fields_ = [("cloud", CloudDesc), ("poses", _vp), ("model_poses", _vp), ("model_depth", _vp), ("model_gradients", _vp), ("systems", _vp),
                ("residual", _vp), ("workspace", _vp), ("Ht", _i), ("Wt", _i), ("min_count", _i), ("n_iters", _i), ("mfx", ctypes.c_double),
                ("mfy", ctypes.c_double), ("mcx", ctypes.c_double), ("mcy", ctypes.c_double), ("max_dist", ctypes.c_double),
                ("max_rot", ctypes.c_double), ("max_trans", ctypes.c_double)]


class NormalsDesc(ctypes.Structure):
    """mirror of s2m2_normals_desc (include/s2m2_hip.h): K28, the normal map of the disparity map"""
    _fields_ = [("cloud", CloudDesc), ("depth", _vp), ("normals", _vp), ("image", _vp), ("count", _vp), ("radius", _i),
                ("max_jump", ctypes.c_double), ("min_cos", ctypes.c_double)]


class SmoothDesc(ctypes.Structure):
    """mirror of s2m2_smooth_desc (include/s2m2_hip.h): K29, edge-preserving smoothing of the disparity map"""
    _fields_ = [("cloud", CloudDesc), ("disp_out", _vp), ("taps", _vp), ("count", _vp), ("radius", _i), ("sigma_s", ctypes.c_double),
                ("sigma_r", ctypes.c_double), ("max_jump", ctypes.c_double)]


class RectifyDesc(ctypes.Structure):
    """mirror of s2m2_rectify_desc (include/s2m2_hip.h): K16, the rectifier in front of the forward"""
    _fields_ = [("src", _vp * 2), ("records", _vp), ("out", _vp), ("maps", _vp), ("n_src", _i), ("n_img", _i), ("Hs", _i), ("Ws", _i),
                ("Hd", _i), ("Wd", _i), ("src_format", _i), ("out_dtype", _i), ("round", _i), ("order", _i)]


# s2m2_rectify: source formats, block orders and the record layout (include/s2m2_hip.h: S2M2_RECTIFY_*)
RECTIFY_SRC_U8_HWC, RECTIFY_SRC_U8_CHW, RECTIFY_SRC_F32_CHW = 0, 1, 2
RECTIFY_ORDER_SAMPLE, RECTIFY_ORDER_TILE = 0, 1
RECTIFY_REC_SRC, RECTIFY_REC_IR, RECTIFY_REC_FX, RECTIFY_REC_K1, RECTIFY_RECORD_FLOATS = 0, 1, 10, 14, 20

EVAL_MAX_THR, EVAL_HIST_BINS, EVAL_CONF_BINS = 8, 1025, 64


class EvalDesc(ctypes.Structure):
    """mirror of s2m2_eval_desc (include/s2m2_hip.h): K18, disparity error statistics against ground truth"""
    _fields_ = [("disp", _vp), ("occ", _vp), ("conf", _vp), ("gt", _vp), ("region", _vp), ("workspace", _vp), ("stats", _vp),
                ("B", _i), ("H", _i), ("W", _i), ("Hp", _i), ("Wp", _i), ("nthr", _i), ("thr", ctypes.c_float * EVAL_MAX_THR),
                ("d1_abs", ctypes.c_float), ("d1_rel", ctypes.c_float), ("gt_min", ctypes.c_float), ("conf_min", ctypes.c_float),
                ("occ_min", ctypes.c_float)]


class AttnPlan(ctypes.Structure):
    """mirror of s2m2_attn_plan (include/s2m2_hip.h): the launch K4's planner decides on"""
    _fields_ = [(n, _i) for n in ("dp", "minw", "ksplit", "nxt", "nyt", "nw", "nblk", "kt", "twopass", "qlds", "deep")] + [("lds_bytes", _ll)]


# the stat block of s2m2_disp_eval in 64-bit words (include/s2m2_hip.h: S2M2_EVAL_*): word offsets inside the ALL / KEPT blocks and inside a
# row of the confidence table, then the offsets of the four blocks
EVAL_N_REGION, EVAL_N_EVAL, EVAL_N_NONFINITE, EVAL_SUM_ABS_Q, EVAL_SUM_SQ_Q, EVAL_D1_BAD, EVAL_BAD, EVAL_BLOCK_WORDS = 0, 1, 2, 3, 4, 5, 6, 14
EVAL_CONF_COUNT, EVAL_CONF_SUM_ABS_Q, EVAL_CONF_BAD, EVAL_CONF_ROW_WORDS = 0, 1, 2, 10
EVAL_ALL, EVAL_KEPT, EVAL_HIST, EVAL_CONF, EVAL_WORDS = 0, 14, 28, 1053, 1693

# name -> (restype, argtypes); must list every symbol declared in include/s2m2_hip.h
ABI_VERSION = 800                     # include/s2m2_hip.h: S2M2_ABI_VERSION (checked in load())

SIGNATURES = {
    "s2m2_version": (_i, []),
    "s2m2_last_error": (ctypes.c_char_p, []),
    "s2m2_ln_corr_kernel_name": (ctypes.c_char_p, [_i, _i, _i]),
    "s2m2_cost_volume": (_i, [ctypes.POINTER(CorrDesc), _vp]),
    "s2m2_plan_begin": (_i, [ctypes.POINTER(_vp)]),
    "s2m2_plan_end": (_i, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_size_t), _i]),
    "s2m2_plan_abort": (_i, [_vp]),
    "s2m2_plan_launches": (_i, [_vp]),
    "s2m2_plan_patches": (_i, [_vp, _i]),
    "s2m2_plan_run": (_i, [_vp, ctypes.POINTER(_vp), _i, _vp]),
    "s2m2_plan_destroy": (_i, [_vp]),
    "s2m2_refine_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "s2m2_plan_save": (_i, [_vp, ctypes.POINTER(EngineRegion), _i, ctypes.POINTER(EngineInfo), ctypes.c_char_p]),
    "s2m2_engine_load": (_i, [ctypes.c_char_p, ctypes.POINTER(_vp)]),
    "s2m2_engine_meta": (_i, [_vp, ctypes.POINTER(EngineInfo)]),
    "s2m2_engine_run": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "s2m2_engine_destroy": (_i, [_vp]),
    "s2m2_pack_frag_elems": (_ll, [ctypes.POINTER(PackDesc)]),
    "s2m2_pack_frag": (_i, [ctypes.POINTER(PackDesc), _vp]),
    "s2m2_event_create": (_i, [ctypes.POINTER(_vp)]),
    "s2m2_event_destroy": (_i, [_vp]),
    "s2m2_event_elapsed_us": (_i, [_vp, _vp, ctypes.POINTER(ctypes.c_float)]),
    "s2m2_sinkhorn_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i, _i]),
    "s2m2_pw_direct_supported": (_i, [_i, _i, _i]),
    "s2m2_pw_direct": (_i, [ctypes.POINTER(PwDesc), _vp]),
    "s2m2_conv_narrow_supported": (_i, [_i, _i, _i, _i, _i, _i]),
    "s2m2_conv_narrow": (_i, [ctypes.POINTER(NarrowDesc), _vp]),
    "s2m2_sinkhorn_regress": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "s2m2_cv_lookup": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _ll, _ll, _ll, _i, _vp]),
    "s2m2_conv2d": (_i, [ctypes.POINTER(ConvDesc), _vp]),
    "s2m2_mlp_chain_supported": (_i, [_i, _i]),
    "s2m2_mlp_chain_frag_supported": (_i, [_i, _i]),
    "s2m2_mlp_fan_supported": (_i, [_i, _i, _i]),
    "s2m2_mlp_chain": (_i, [ctypes.POINTER(ChainDesc), _vp]),
    "s2m2_conv_block_supported": (_i, [_i, _i, _i, _i]),
    "s2m2_conv_block": (_i, [ctypes.POINTER(ConvBlockDesc), _vp]),
    "s2m2_conv_gru_supported": (_i, [_i, _i, _i, _i]),
    "s2m2_conv_gru": (_i, [ctypes.POINTER(ConvGruDesc), _vp]),
    "s2m2_conv_block_tail_supported": (_i, [_i, _i, _i, _i]),
    "s2m2_conv_block_tail": (_i, [ctypes.POINTER(ConvTailDesc), _vp]),
    "s2m2_row_attn_supported": (_i, [_i, _i, _i, _i]),
    "s2m2_row_attn": (_i, [ctypes.POINTER(RowAttnDesc), _vp]),
    "s2m2_feature_fusion_supported": (_i, [_i, _i]),
    "s2m2_feature_fusion": (_i, [_vp, _vp, _vp, _ll, _ll, _ll, _ll, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "s2m2_feature_fusion_frag_supported": (_i, [_i, _i]),
    "s2m2_feature_fusion_frag": (_i, [_vp, _vp, _vp, _ll, _ll, _ll, _ll, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "s2m2_convex_upsample": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _ll, _i, _vp]),
    "s2m2_attention": (_i, [_vp, _vp, _vp, _vp, _ll, _ll, _ll, _ll, _i, _i, _i, _i, _i, ctypes.c_float, _i, _vp, _vp, _vp, _ll,
                            _i, _i, _i, _vp]),
    "s2m2_attention_supported": (_i, [_i, _i, _i, _i, _i, _i, _i]),
    "s2m2_attention_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, ctypes.POINTER(AttnPlan)]),
    "s2m2_resample2x": (_i, [_vp, _vp, _i, _i, _i, _i, _ll, _ll, _i, _i, _vp]),
    "s2m2_image_prep": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "s2m2_refine_prep": (_i, [_vp, _vp, _vp, _vp, _ll, _i, _i, _vp]),
    "s2m2_global_update": (_i, [_vp, _i, _vp, _vp, _vp, _ll, _i, _i, _vp]),
    "s2m2_refine_update": (_i, [_vp, _i, _vp, _vp, _vp, _ll, _i, _i, _i, _vp]),
    "s2m2_debug_poison_lds": (_i, [_vp]),
    "s2m2_debug_clock_probe": (_i, [_vp, _vp]),
    "s2m2_refine_update_to": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _vp]),
    "s2m2_tanh": (_i, [_vp, _vp, _ll, _i, _vp]),
    "s2m2_stem_mlp": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _vp]),
    "s2m2_image_pad": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "s2m2_layernorm": (_i, [_vp, _vp, _ll, _i, _ll, _ll, _i, _vp]),
    "s2m2_groupnorm_workspace_bytes": (ctypes.c_size_t, [_i, _i]),
    "s2m2_groupnorm_nhwc": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _ll, _i, _i, ctypes.c_float, _i, _vp]),
    "s2m2_cloud_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "s2m2_cloud": (_i, [ctypes.POINTER(CloudDesc), _vp]),
    "s2m2_rectify": (_i, [ctypes.POINTER(RectifyDesc), _vp]),
    "s2m2_eval_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "s2m2_eval_tile_rows": (_i, [_i, _i]),
    "s2m2_disp_eval": (_i, [ctypes.POINTER(EvalDesc), _vp]),
    "s2m2_mesh_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "s2m2_mesh_tile_rows": (_i, [_i, _i]),
    "s2m2_mesh": (_i, [ctypes.POINTER(MeshDesc), _vp]),
    "s2m2_register_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "s2m2_register": (_i, [ctypes.POINTER(RegisterDesc), _vp]),
    "s2m2_segment_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "s2m2_segment_tile_rows": (_i, [_i, _i]),
    "s2m2_segment_tile_cols": (_i, [_i, _i]),
    "s2m2_segment": (_i, [ctypes.POINTER(SegmentDesc), _vp]),
    "s2m2_voxel_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i, _ll]),
    "s2m2_voxel_tile_rows": (_i, [_i, _i]),
    "s2m2_voxel_home_slot": (_ll, [_i, _i, _i, _ll]),
    "s2m2_voxel": (_i, [ctypes.POINTER(VoxelDesc), _vp]),
    "s2m2_tsdf_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "s2m2_tsdf_tile_voxels": (_i, [_i, _i, _i]),
    "s2m2_tsdf_integrate": (_i, [ctypes.POINTER(TsdfDesc), _vp]),
    "s2m2_tsdf_extract": (_i, [ctypes.POINTER(TsdfExtractDesc), _vp]),
    "s2m2_tsdf_mesh_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "s2m2_tsdf_mesh": (_i, [ctypes.POINTER(TsdfMeshDesc), _vp]),
    "s2m2_tsdf_raycast": (_i, [ctypes.POINTER(TsdfRaycastDesc), _vp]),
    "s2m2_tsdf_track_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "s2m2_tsdf_track": (_i, [ctypes.POINTER(TsdfTrackDesc), _vp]),
    "s2m2_normals": (_i, [ctypes.POINTER(NormalsDesc), _vp]),
    "s2m2_smooth": (_i, [ctypes.POINTER(SmoothDesc), _vp]),
    "s2m2_smooth_weights": (_i, [_i, ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                                 ctypes.POINTER(ctypes.c_float)]),
}


def load() -> ctypes.CDLL:
    """dlopen the kernel library (once).  Raises if it has not been built (python -m s2m2_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not found: build it with `python -m s2m2_amd.build` "
                               "(the S2M2 hot path has no PyTorch fallback)")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:                    # a stale library of the same ABI version (additive entry points do not bump it)
                raise RuntimeError(f"{LIB_PATH} does not export {name} (include/s2m2_hip.h): "
                                   "rebuild the library with `python -m s2m2_amd.build`") from None
            fn.restype = res
            fn.argtypes = args
        ver = lib.s2m2_version()
        if ver != ABI_VERSION:                        # exact: descriptor layouts change in place between patch versions as well
            raise RuntimeError(f"{LIB_PATH} reports ABI version {ver}, this binding was written against {ABI_VERSION} "
                               "(include/s2m2_hip.h: S2M2_ABI_VERSION): rebuild the library with `python -m s2m2_amd.build`")
        _lib = lib
    return _lib


# Optional work meter (bench.py): family -> [flops, launches] of the multiply-accumulate work the launches execute (padded channel
# counts, 2 flops per MAC); ATTN_EVENTS: list collecting (start event, end event, flops, shape tag) around every K4 launch.
METER: Optional[dict] = None
ATTN_EVENTS: Optional[list] = None
ROW_EVENTS: Optional[list] = None     # like ATTN_EVENTS around every K13 launch: (start, end, flops, unique HBM bytes, shape tag)


def _meter(family: str, flops: float) -> None:
    if METER is not None:
        e = METER.setdefault(family, [0.0, 0])
        e[0] += flops
        e[1] += 1


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed: {load().s2m2_last_error().decode()}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# ---- operand validation.  The C ABI sees raw pointers and integers, so this is the only place that can check what a pointer stands for.
# A wrapper reads as: residency of all its operands (_resident, once), geometry of each operand (one helper call each: pure functions of
# shape, stride and dtype, so they run on CPU tensors too), descriptor, launch.

def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def _ptrs(ts):
    """ctypes array of the base pointers of ``ts`` (None -> NULL; never empty, so that it always has an address)"""
    return (_vp * max(len(ts), 1))(*[_ptr(t) for t in ts])


def _resident(what: str, *ts: Optional[torch.Tensor]) -> None:
    """every tensor a kernel will dereference lives on the GPU, all on the same one (None: an absent optional operand)"""
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError(f"{what}: operands must be device tensors, got one on {t.device}")
        if dev is not None and t.device != dev:
            raise ValueError(f"{what}: operands must be device tensors on one device, got {dev} and {t.device}")
        dev = t.device


def _contig(what: str, *ts: Optional[torch.Tensor]) -> None:
    """operands the kernel indexes as one dense block"""
    for t in ts:
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{what}: tensors must be contiguous, got shape {tuple(t.shape)} strides {t.stride()}")


def _rows(x: torch.Tensor, what: str):
    """(rows, row stride) of a (..., C) tensor with contiguous channels and a uniform row stride (a channel slice of a wider tensor is fine)"""
    C = x.shape[-1]
    if x.stride(-1) != 1:
        raise ValueError(f"{what}: channels must be contiguous")
    xs = x.stride(-2) if x.dim() > 1 else C
    for d in range(x.dim() - 2):
        if x.shape[d] > 1 and x.stride(d) != x.stride(d + 1) * x.shape[d + 1]:
            raise ValueError(f"{what}: rows must have a uniform stride")
    return x.numel() // C, xs


def _pixels(t: torch.Tensor, what: str) -> int:
    """pixel stride of an (N,H,W,C) view, channels contiguous, pixels dense with a common pixel stride (a channel slice of a wider tensor is fine)"""
    if t.dim() != 4 or t.stride(3) != 1:
        raise ValueError(f"{what}: expected an (N,H,W,C) tensor with contiguous channels, got {tuple(t.shape)} {t.stride()}")
    n, h, w, c = t.shape
    ps = t.stride(2)
    if (h > 1 and t.stride(1) != w * ps) or (n > 1 and t.stride(0) != h * w * ps):
        raise ValueError(f"{what}: pixels are not dense: shape {tuple(t.shape)} strides {t.stride()}")
    return ps


def _cv_pitch(cv: torch.Tensor, what: str) -> int:
    """(B,h,w,w) cost volume, columns contiguous, volume rows ``pitch`` elements apart (a padded allocation viewed ``[..., :w]``, or
    plain contiguous: pitch = w), image rows and batch entries dense behind that."""
    if cv.dim() != 4 or cv.shape[2] != cv.shape[3]:
        raise ValueError(f"{what}: cv must be a (B,h,w,w) tensor, got {tuple(cv.shape)}")
    B, h, w, _ = cv.shape
    pitch = cv.stride(2)
    if cv.stride(3) != 1 or pitch < w or pitch % 8 or (h > 1 and cv.stride(1) != w * pitch) or (B > 1 and cv.stride(0) != h * w * pitch):
        raise ValueError(f"{what}: cv strides {cv.stride()} are not a row-padded (B,h,w,w) volume")
    return pitch


def _lookup_geometry(what: str, cv: torch.Tensor, disp: torch.Tensor, radius: int, buf: Optional[torch.Tensor] = None,
                     off1: int = 0, off2: int = 0) -> int:
    """the operands of K3 (s2m2_cv_lookup): cv a (B,h,w,w) fp16 / fp32 volume (_cv_pitch, returned), disp its contiguous fp32 (B,1,h,w)
    map -- the kernel reads it through a float pointer whatever it holds --, 0 <= radius <= 16; and, writing into channel slots of a wider
    tensor, buf contiguous (B,h,w,Cb) fp16 / fp32 with the 2r+1 channels at off1 and those at off2 inside a pixel and apart from each other."""
    pitch = _cv_pitch(cv, what)
    B, h, w, _ = cv.shape
    if cv.dtype not in _DT:
        raise ValueError(f"{what}: cv must be fp16 or fp32, got {cv.dtype}")
    if not isinstance(radius, int) or not 0 <= radius <= 16:
        raise ValueError(f"{what}: radius must be an integer in [0, 16], got {radius!r}")
    _mat(disp, (B, 1, h, w), torch.float32, f"{what}: disp")
    if buf is not None:
        T = 2 * radius + 1
        if buf.dim() != 4 or tuple(buf.shape[:3]) != (B, h, w) or buf.dtype not in _DT or not buf.is_contiguous():
            raise ValueError(f"{what}: buf must be a contiguous ({B}, {h}, {w}, Cb) fp16 or fp32 tensor, got {tuple(buf.shape)} {buf.dtype} "
                             f"strides {buf.stride()}")
        cb = buf.shape[3]
        for name, off in (("off1", off1), ("off2", off2)):
            if not isinstance(off, int) or not 0 <= off <= cb - T:
                raise ValueError(f"{what}: {name}={off!r}: the {T} taps must lie inside the {cb} channels of a pixel")
        if abs(off1 - off2) < T:
            raise ValueError(f"{what}: the tap ranges at off1={off1} and off2={off2} ({T} channels each) overlap")
    return pitch


def _vec(t: Optional[torch.Tensor], n: int, what: str, *, at_least: bool = False, dtype: torch.dtype = torch.float32,
         optional: bool = False) -> None:
    """a contiguous block of exactly ``n`` elements of ``dtype`` (at_least: ``n`` or more, the padded biases of K11 / K12); optional: None passes"""
    if t is None:
        if optional:
            return
        raise ValueError(f"{what} is missing")
    if t.dtype != dtype or not t.is_contiguous() or (t.numel() < n if at_least else t.numel() != n):
        raise ValueError(f"{what} must be a contiguous {dtype} vector of {'at least ' if at_least else ''}{n} elements, "
                         f"got {tuple(t.shape)} {t.dtype} strides {t.stride()}")


def _mat(t: torch.Tensor, shape, dtype: torch.dtype, what: str) -> None:
    """a contiguous tensor of exactly this shape and dtype"""
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {tuple(shape)} {dtype} tensor, got {tuple(t.shape)} {t.dtype} strides {t.stride()}")


def _frag(t: torch.Tensor, cout: int, k: int, dtype: torch.dtype, what: str) -> None:
    """the MFMA-fragment stream of a (cout, k) matrix: 32-row x 16-column tiles of 64 lanes x 8 values (pack.pw_frag / pack.narrow_frag)"""
    _mat(t, ((cout + 31) // 32, (k + 15) // 16, 64, 8), dtype, f"{what} of a ({cout}, {k}) matrix")


@contextlib.contextmanager
def _bracket(events: Optional[list], *fields):
    """the optional event pair around one launch (ATTN_EVENTS / ROW_EVENTS): appends (start, stop, *fields) once the launch went through"""
    if events is None:
        yield
        return
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    yield
    ev[1].record()
    events.append(ev + fields)


def pack_frag(kind: int, w: torch.Tensor, w2: Optional[torch.Tensor] = None, ntap: int = 1, rows: Optional[int] = None) -> torch.Tensor:
    """s2m2_pack_frag: the plain packing ``w`` (rows, K) fp16 on the device -> flat fp16 tensor holding the fragment stream of the direct-form
    kernel named by ``kind`` (PACK_ROWS / PACK_NARROW / PACK_CONV_FRAG / PACK_FUSION / PACK_HEAD; include/s2m2_hip.h).  One-time set-up."""
    _resident("pack_frag", w, w2)
    d = PackDesc()
    for name, t in (("w", w), ("w2", w2)):
        if t is not None and (t.dtype != torch.float16 or t.dim() != 2):
            raise ValueError(f"pack_frag: {name} must be a 2-D fp16 device tensor with contiguous rows")
    d.w, d.ld = w.data_ptr(), _rows(w, "pack_frag: w")[1]
    if w2 is not None:
        d.w2, d.ld2 = w2.data_ptr(), _rows(w2, "pack_frag: w2")[1]
    d.kind, d.rows, d.cols, d.ntap = kind, rows if rows is not None else w.shape[0], w.shape[1], ntap
    lib = load()
    n = lib.s2m2_pack_frag_elems(ctypes.byref(d))
    if n < 0:
        raise RuntimeError(f"s2m2_pack_frag_elems failed: {lib.s2m2_last_error().decode()}")
    out = torch.empty(n, device=w.device, dtype=torch.float16)
    d.out, d.out_elems = out.data_ptr(), n
    with torch.cuda.device(w.device):
        _check(lib.s2m2_pack_frag(ctypes.byref(d), _stream()), "s2m2_pack_frag")
    return out


class Plan:
    """A recorded launch plan (s2m2_plan_*): ``with Plan.record(externals) as p: ...`` records every library call this thread makes inside the
    block (they run as always); afterwards ``p.run(externals)`` re-issues the sequence natively with the external tensors somewhere else.
    externals: list of tensors (or None).  The tensors allocated inside the block must be kept alive by the caller (engine: a private MemPool)."""

    def __init__(self):
        self.h = _vp()
        self.n = 0
        self.sealed = False

    class _Rec:
        def __init__(self, plan, externals):
            self.plan, self.ext = plan, externals

        def __enter__(self):
            _check(load().s2m2_plan_begin(ctypes.byref(self.plan.h)), "s2m2_plan_begin")
            return self.plan

        def __exit__(self, et, ev, tb):
            lib = load()
            if et is not None:
                lib.s2m2_plan_abort(self.plan.h)
                return False
            n = len(self.ext)
            size = (ctypes.c_size_t * max(n, 1))(*[(t.numel() * t.element_size() if t is not None else 0) for t in self.ext])
            _check(lib.s2m2_plan_end(self.plan.h, _ptrs(self.ext), size, n), "s2m2_plan_end")
            self.plan.n, self.plan.sealed = n, True
            return False

    def record(self, externals):
        return Plan._Rec(self, externals)

    @property
    def launches(self) -> int:
        return load().s2m2_plan_launches(self.h)

    def patches(self, slot: int = -1) -> int:
        return load().s2m2_plan_patches(self.h, slot)

    def run(self, externals) -> None:
        _check(load().s2m2_plan_run(self.h, _ptrs(externals), len(externals), _stream()), "s2m2_plan_run")

    def refine_step(self, hidden, ctx, disp, conf, occ, cv, side) -> None:
        """s2m2_refine_step: this plan as one refinement iteration, externals in the ABI's fixed order"""
        _check(load().s2m2_refine_step(self.h, *_ptrs((hidden, ctx, disp, conf, occ, cv, side)), _stream()), "s2m2_refine_step")

    def __del__(self):
        try:
            if self.h:
                load().s2m2_plan_destroy(self.h)
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


class KernelTimer:
    """A start / stop HIP event pair attached to ONE kernel dispatch (s2m2_corr_desc.start_event / stop_event): elapsed_us() is the kernel's own execution
    time, what a rocprofv3 kernel trace reports, without the dispatch gaps that events recorded around a launch include."""

    def __init__(self):
        self.start, self.stop = _vp(), _vp()
        _check(load().s2m2_event_create(ctypes.byref(self.start)), "s2m2_event_create")
        _check(load().s2m2_event_create(ctypes.byref(self.stop)), "s2m2_event_create")

    def elapsed_us(self) -> float:
        us = ctypes.c_float()
        _check(load().s2m2_event_elapsed_us(self.start, self.stop, ctypes.byref(us)), "s2m2_event_elapsed_us")
        return float(us.value)

    def __del__(self):
        try:
            load().s2m2_event_destroy(self.start)
            load().s2m2_event_destroy(self.stop)
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def _cost_volume(tokens: torch.Tensor, ln, cv_dtype, out, timer, band: int, what: str) -> torch.Tensor:
    """one launch of K1 through its descriptor (s2m2_cost_volume); ln = (weight, bias) or None (tokens normalised already).  Without ``out`` the
    volume is allocated plain (ln: the form ln_corr always returned) or with row-padded lines (cv_alloc)."""
    ln = ln or ()
    _resident(what, tokens, *ln, out)
    _contig(what, tokens, *ln)
    twoB, h, w, C = tokens.shape
    B = twoB // 2
    if out is not None:
        cv = out
    elif ln:
        cv = torch.empty((B, h, w, w), device=tokens.device, dtype=cv_dtype or tokens.dtype)
    else:
        cv = cv_alloc(B, h, w, cv_dtype or tokens.dtype, tokens.device)
    if tuple(cv.shape) != (B, h, w, w):
        raise ValueError(f"{what}: out must be a (B,h,w,w) tensor")
    d = CorrDesc()
    d.tokens, d.cv = tokens.data_ptr(), cv.data_ptr()
    keep = [t.float().contiguous() for t in ln]
    if keep:
        d.ln_weight, d.ln_bias = keep[0].data_ptr(), keep[1].data_ptr()
    d.B, d.h, d.w, d.C = B, h, w, C
    d.cv_pitch, d.band = _cv_pitch(cv, what), band if band >= 0 else -1
    d.token_dtype, d.cv_dtype = _DT[tokens.dtype], _DT[cv.dtype]
    if timer is not None:
        d.start_event, d.stop_event = timer.start, timer.stop
    _check(load().s2m2_cost_volume(ctypes.byref(d), _stream()), "s2m2_cost_volume")
    _meter("ln_corr", 2.0 * B * h * w * w * C)
    return cv


def ln_corr(feat: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, cv_dtype: Optional[torch.dtype] = None,
            out: Optional[torch.Tensor] = None, timer: Optional[KernelTimer] = None, band: int = -1) -> torch.Tensor:
    """feat (2B,h,w,C) channels-last tokens (left = first B) -> cv (B,h,w,w), LayerNorm inside the kernel.  [A4]   timer: see KernelTimer.
    band >= 0: only columns j <= i + band are written, the rest of ``cv`` keeps whatever it held.  ``out`` may be a row-padded view (cv_alloc)."""
    return _cost_volume(feat, (ln_w, ln_b), cv_dtype, out, timer, band, "ln_corr")


def cv_alloc(B: int, h: int, w: int, dtype: torch.dtype, device, aligned: bool = True) -> torch.Tensor:
    """(B,h,w,w) cost volume whose rows start on 128-byte lines: allocated (B,h,w,pitch) with pitch = w rounded up to 128 bytes and
    returned as the ``[..., :w]`` view (K1's 64-column store granules are then whole lines: no partial-line writes)."""
    per = 128 // (2 if dtype == torch.float16 else 4)
    pitch = (w + per - 1) // per * per if aligned else w
    return torch.empty((B, h, w, pitch), device=device, dtype=dtype)[..., :w]


def corr(tokens: torch.Tensor, cv_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None,
         timer: Optional[KernelTimer] = None, band: int = -1) -> torch.Tensor:
    """tokens (2B,h,w,C) ALREADY LayerNorm'ed (left = first B) -> cv (B,h,w,w), a row-padded view (cv_alloc) unless ``out`` is given.
    [A4 without the LayerNorm: s2m2_cost_volume with ln_weight = NULL]"""
    return _cost_volume(tokens, None, cv_dtype, out, timer, band, "corr")


def sinkhorn_regress(cv: torch.Tensor, use_positivity: bool, ot_iter: int = 3, want_argmax: bool = False):
    """cv (B,h,w,w) (row-padded views accepted) -> disp, conf, occ (B,1,h,w) fp32 [, argmax (B,h,w) int32].  [A5+A6]"""
    _resident("sinkhorn_regress", cv)
    pitch = _cv_pitch(cv, "sinkhorn_regress")
    B, h, w, _ = cv.shape
    out = torch.empty((3, B, 1, h, w), device=cv.device, dtype=torch.float32)
    am = torch.empty((B, h, w), device=cv.device, dtype=torch.int32) if want_argmax else None
    _check(load().s2m2_sinkhorn_regress(cv.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), _ptr(am), B, h, w, ot_iter,
                                        int(use_positivity), _DT[cv.dtype], pitch, None, _stream()), "s2m2_sinkhorn_regress")
    return (out[0], out[1], out[2], am) if want_argmax else (out[0], out[1], out[2])


def cv_lookup(cv: torch.Tensor, disp: torch.Tensor, radius: int = 4, channels_last: bool = False,
              out_dtype: torch.dtype = torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """cv (B,h,w,w), disp (B,1,h,w) fp32 -> corr1, corr2: (B,2r+1,h,w) planar or (B,h,w,2r+1) channels-last.  [A9+A10]"""
    _resident("cv_lookup", cv, disp)
    pitch = _lookup_geometry("cv_lookup", cv, disp, radius)
    if out_dtype not in _DT:
        raise ValueError(f"cv_lookup: out_dtype must be fp16 or fp32, got {out_dtype}")
    B, h, w, _ = cv.shape
    T = 2 * radius + 1
    if channels_last:
        both = torch.empty((B, h, w, 2 * T), device=cv.device, dtype=out_dtype)
        c1, c2 = both[..., :T], both[..., T:]
        bs, ps, ts = h * w * 2 * T, 2 * T, 1
    else:
        both = torch.empty((2, B, T, h, w), device=cv.device, dtype=out_dtype)
        c1, c2 = both[0], both[1]
        bs, ps, ts = T * h * w, 1, h * w
    _check(load().s2m2_cv_lookup(cv.data_ptr(), disp.data_ptr(), c1.data_ptr(), c2.data_ptr(), B, h, w, radius,
                                 _DT[cv.dtype], _DT[out_dtype], bs, ps, ts, pitch, _stream()), "s2m2_cv_lookup")
    return c1, c2


def conv2d(srcs, weight: torch.Tensor, bias: Optional[torch.Tensor], KH: int, KW: int, Cout: int, act: int = ACT_NONE,
           epi: int = EPI_NONE, aux0: Optional[torch.Tensor] = None, aux1: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None, out_scale: float = 1.0, shuffle2: int = 0, tile: int = 0,
           stride: int = 1, korder: int = 0, ln_wsum: Optional[torch.Tensor] = None, ln_eps: float = 1e-5,
           ksplit: int = 0, bias2: Optional[torch.Tensor] = None, pool2: bool = False, epi_cout0: int = 0) -> torch.Tensor:
    """Implicit-GEMM convolution / linear layer (s2m2_conv2d).  srcs: list of (N,H,W,Cs) tensors, concatenated along C;
    weight: packed (Cout, KH*KW*sum(Cs)) (see s2m2_amd.pack); bias fp32 (Cout) or None.  Returns (N,H,W,Cout), or
    (N,2H,2W,shuffle2) for the 2x2-stride-2 transposed-conv GEMM.  ln_wsum (fp32 (Cout) row sums of the packed weight): the 1x1 layer
    is preceded by LayerNorm(Cin, no affine, eps=ln_eps) of the raw input rows, folded into the kernel.  pool2: the 1x1 layer is preceded
    by AvgPool2d(2), folded into its operand load -> (N, H//2, W//2, Cout).  epi_cout0 > 0: the one-operand epilogue applies to couts
    >= epi_cout0 only and aux0 has Cout - epi_cout0 channels (two stacked layers, one launch: s2m2_conv_desc.epi_cout0)."""
    if isinstance(srcs, torch.Tensor):
        srcs = [srcs]
    if pool2 and (KH, KW, stride) != (1, 1, 1):      # the output grid below is only that of AvgPool2d(2) + 1x1; refused like the library refuses it
        raise RuntimeError("conv2d: pool2 needs a plain 1x1 stride-1 layer")
    _resident("conv2d", *srcs, weight, bias, aux0, aux1, out, ln_wsum, bias2)
    d = ConvDesc()
    x0 = srcs[0]
    n, h, w, _ = x0.shape
    dt = x0.dtype
    cin = 0
    for i, t in enumerate(srcs):
        if t.dtype != dt or tuple(t.shape[:3]) != (n, h, w):
            raise ValueError("conv2d: sources must share dtype and (N,H,W)")
        d.src[i], d.src_c[i], d.src_stride[i] = t.data_ptr(), t.shape[3], _pixels(t, "conv2d: source")
        cin += t.shape[3]
    ck = 192 if (Cout % 128 != 0 and Cout % 192 == 0 and cin % 192 == 0) else 128        # s2m2_conv_frag_chunk
    kcols = KH * KW * (-(-cin // ck) * ck) if korder == 2 else KH * KW * cin           # K order 2: K padded to whole chunks
    _mat(weight, (Cout, kcols), dt, "conv2d: packed weight")
    _vec(bias, Cout, "conv2d: bias", optional=True)
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    if pool2:
        ho, wo = h // 2, w // 2
    exp_shape = (n, 2 * h, 2 * w, shuffle2) if shuffle2 else (n, ho, wo, Cout)
    if out is None:
        out = torch.empty(exp_shape, device=x0.device, dtype=dt)
    if tuple(out.shape) != exp_shape or out.dtype != dt:
        raise ValueError(f"conv2d: out must be {exp_shape} {dt}, got {tuple(out.shape)} {out.dtype}")
    d.nsrc = len(srcs)
    d.weight, d.bias, d.out, d.out_stride = weight.data_ptr(), _ptr(bias), out.data_ptr(), _pixels(out, "conv2d: out")
    d.N, d.H, d.W, d.KH, d.KW, d.Cout = n, h, w, KH, KW, Cout
    d.act, d.epi = act, epi
    for name, a, ac in (("aux0", aux0, Cout - epi_cout0), ("aux1", aux1, Cout)):
        if a is not None and (a.dtype != dt or tuple(a.shape) != (n, ho, wo, ac)):
            raise ValueError(f"conv2d: {name} must be {(n, ho, wo, ac)} {dt}, got {tuple(a.shape)} {a.dtype}")
    if aux0 is not None:                   # (aux0 of an epi_cout0 launch: its own base; the library applies the cout offset)
        d.aux0, d.aux0_stride = aux0.data_ptr(), _pixels(aux0, "conv2d: aux0")
    if aux1 is not None:
        d.aux1, d.aux1_stride = aux1.data_ptr(), _pixels(aux1, "conv2d: aux1")
    d.epi_cout0, d.out_scale, d.shuffle2 = epi_cout0, out_scale, shuffle2
    d.tile, d.stride, d.korder, d.pool2 = tile, stride, korder, int(pool2)
    if ln_wsum is not None:
        _vec(ln_wsum, Cout, "conv2d: ln_wsum")
        d.ln_wsum, d.ln_eps = ln_wsum.data_ptr(), ln_eps
    if epi == EPI_DUALMIX:
        _vec(bias2, Cout, "conv2d: bias2", optional=True)
        d.ksplit, d.bias2 = ksplit, _ptr(bias2)
    d.dtype = _DT[dt]
    _check(load().s2m2_conv2d(ctypes.byref(d), _stream()), "s2m2_conv2d")
    _meter("conv2d", 2.0 * n * ho * wo * Cout * KH * KW * cin)
    return out


def mlp_chain_supported(C: int, dtype: torch.dtype) -> bool:
    return bool(load().s2m2_mlp_chain_supported(C, _DT[dtype]))


def mlp_fan_supported(C: int, nfan: int, dtype: torch.dtype) -> bool:
    return bool(load().s2m2_mlp_fan_supported(C, nfan, _DT[dtype]))


def _chain_input(d: ChainDesc, x: torch.Tensor, pool2: bool, what: str):
    """the x / rows / pool fields of a chain descriptor -> (rows, leading shape of the outputs); pool2: x (N,H,W,C) is read through AvgPool2d(2)"""
    rows, xs = _rows(x, what)
    oshape = tuple(x.shape[:-1])
    if pool2:
        oshape = (x.shape[0], x.shape[1] // 2, x.shape[2] // 2)
        rows = oshape[0] * oshape[1] * oshape[2]
        d.pool_h, d.pool_w = x.shape[1], x.shape[2]
    d.x, d.x_stride, d.rows, d.C, d.dtype = x.data_ptr(), xs, rows, x.shape[-1], _DT[x.dtype]
    return rows, oshape


def _chain_fan(d: ChainDesc, x: torch.Tensor, oshape, weight: torch.Tensor, bias, ln_wsum, what: str):
    """the fan block of a chain descriptor: n stacked C -> C layers, packed (n*C, C), on the rows the launch produces -> (fan_out (..., n*C), n)"""
    C = x.shape[-1]
    n = weight.shape[0] // C
    _mat(weight, (n * C, C), x.dtype, f"{what}: fan weight, packed (n*{C}, {C}),")
    _vec(bias, n * C, f"{what}: fan bias", optional=True)
    _vec(ln_wsum, n * C, f"{what}: fan ln_wsum", optional=True)
    out = torch.empty(oshape + (n * C,), device=x.device, dtype=x.dtype)
    d.fan_weight, d.fan_out, d.fan_out_stride, d.nfan = weight.data_ptr(), out.data_ptr(), n * C, n
    d.fan_bias, d.fan_ln_wsum = _ptr(bias), _ptr(ln_wsum)
    return out, n


def mlp_fan(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], ln_wsum: Optional[torch.Tensor], ln_eps: float = 1e-5,
            frag: bool = True, pool2: bool = False) -> torch.Tensor:
    """n stacked C -> C layers on the rows of x (..., C) -> (..., n*C) in one pass over the rows (s2m2_mlp_chain with nstage = 0: the
    fan-out-only launch of the direct form; pre-LayerNorm folded in when ln_wsum is given).  weight (n*C, C) in MFMA-fragment order
    (pack.chain_frag; mlp_fan_supported: fp16, C = 128 / 256, any row count, n <= 4).  pool2 (x (N,H,W,C)): nn.AvgPool2d(2) in front of
    the layers, folded into the tile load -> (N, H//2, W//2, n*C)."""
    if not frag:
        raise ValueError("mlp_fan: the fan-out-only launch exists in the direct form only (weight in fragment order, frag=True)")
    _resident("mlp_fan", x, weight, bias, ln_wsum)
    if pool2 and (x.dim() != 4 or x.shape[1] < 2 or x.shape[2] < 2):
        raise ValueError("mlp_fan: pool2 needs frag and an (N,H,W,C) tensor of at least 2x2 pixels")
    C = x.shape[-1]
    d = ChainDesc()
    rows, oshape = _chain_input(d, x, pool2, "mlp_fan")
    d.nstage, d.ln_eps, d.res_stage, d.weight_frag = 0, ln_eps, -1, 1
    out, n = _chain_fan(d, x, oshape, weight, bias, ln_wsum, "mlp_fan")
    _check(load().s2m2_mlp_chain(ctypes.byref(d), _stream()), "s2m2_mlp_chain")
    _meter("mlp_chain", 2.0 * rows * C * C * n)
    return out


def mlp_chain_frag_supported(C: int, dtype: torch.dtype) -> bool:
    """the direct form of mlp_chain (weights in MFMA-fragment order, pack.chain_frag) exists for this width"""
    return bool(load().s2m2_mlp_chain_frag_supported(C, _DT[dtype]))


def mlp_chain_ln_out_supported(C: int, dtype: torch.dtype) -> bool:
    """the optional LayerNorm output of mlp_chain needs a row of 8 k <= 64 16-byte pieces, in either form of the kernel"""
    ppr = C * (2 if dtype == torch.float16 else 4) // 16
    return (mlp_chain_supported(C, dtype) or mlp_chain_frag_supported(C, dtype)) and ppr % 8 == 0 and ppr <= 64


def mlp_chain(x: torch.Tensor, stages, res: Optional[torch.Tensor] = None, res_stage: int = -1, carry: bool = False,
              ln_eps: float = 1e-5, ln_out: Optional[Tuple[torch.Tensor, torch.Tensor, float]] = None, xcd_group_rows: int = 0,
              fan=None, frag: bool = False, pool2: bool = False):
    """Up to three C -> C 1x1 layers on the rows of x (..., C) in one launch (s2m2_mlp_chain).  stages: list of
    (packed weight (C, C), fp32 bias (C) or None, activation, ln_wsum fp32 (C) or None = pre-LayerNorm of that stage's input);
    res (same shape as x) is added to the output of stage res_stage; carry adds the output of stage 0 to the last of 3 stages.
    ln_out = (gamma fp32 (C), beta fp32 (C), eps): also return LayerNorm(out) * gamma + beta  -> (out, normalised).
    xcd_group_rows: placement hint (s2m2_chain_desc): x is images of 8 groups of that many rows, group g runs on XCD g.
    fan = (packed weight (n*C, C), fp32 bias (n*C) or None, ln_wsum fp32 (n*C) or None): n further C -> C layers on the OUTPUT rows
    (pre-LayerNorm folded in when ln_wsum is given), returned as one (..., n*C) tensor: the fused QKV projection of the next attention.
    frag: every weight (stages and fan) is in MFMA-fragment order (pack.chain_frag) -> the direct form of the kernel, meant for short row
    counts (mlp_chain_frag_supported).  pool2 (frag, x (N,H,W,C), no res / carry / ln_out): nn.AvgPool2d(2) in front of the first stage,
    folded into the tile load -> outputs on the (N, H//2, W//2) grid.
    Return value: out, or a tuple (out[, normalised][, fan_out]) in that order."""
    _resident("mlp_chain", x, res, *[t for w, b, _, wsum in stages for t in (w, b, wsum)], *(ln_out[:2] if ln_out is not None else ()),
              *(fan or ()))
    if pool2 and (not frag or x.dim() != 4 or x.shape[1] < 2 or x.shape[2] < 2 or res_stage >= 0 or carry or ln_out is not None):
        raise ValueError("mlp_chain: pool2 needs frag, an (N,H,W,C) tensor of at least 2x2 pixels and no res / carry / ln_out")
    if not 1 <= len(stages) <= 3:
        raise ValueError("mlp_chain: 1..3 stages")
    C = x.shape[-1]
    d = ChainDesc()
    rows, oshape = _chain_input(d, x, pool2, "mlp_chain")
    d.nstage = len(stages)
    for i, (w, b, act, wsum) in enumerate(stages):
        _mat(w, (C, C), x.dtype, f"mlp_chain: packed weight[{i}]")
        _vec(b, C, f"mlp_chain: bias[{i}]", optional=True)
        _vec(wsum, C, f"mlp_chain: ln_wsum[{i}]", optional=True)
        d.weight[i], d.act[i], d.bias[i], d.ln_wsum[i] = w.data_ptr(), act, _ptr(b), _ptr(wsum)
    d.res_stage, d.carry, d.ln_eps = res_stage, int(carry), ln_eps
    d.xcd_group_rows = int(xcd_group_rows)
    d.weight_frag = int(bool(frag))
    if res_stage >= 0:
        if res is None or res.dtype != x.dtype or tuple(res.shape) != tuple(x.shape):
            raise ValueError("mlp_chain: res must match x")
        d.res, d.res_stride = res.data_ptr(), _rows(res, "mlp_chain: res")[1]
    out = torch.empty(oshape + (C,), device=x.device, dtype=x.dtype)
    d.out, d.out_stride = out.data_ptr(), C
    normed = None
    if ln_out is not None:
        gam, bet, eps = ln_out
        _vec(gam, C, "mlp_chain: ln_out gamma")
        _vec(bet, C, "mlp_chain: ln_out beta")
        normed = torch.empty(x.shape, device=x.device, dtype=x.dtype)
        d.ln_out, d.ln_out_stride, d.ln_gamma, d.ln_beta, d.ln_out_eps = normed.data_ptr(), C, gam.data_ptr(), bet.data_ptr(), float(eps)
    fan_out, nfan = _chain_fan(d, x, oshape, *fan, "mlp_chain") if fan is not None else (None, 0)
    _check(load().s2m2_mlp_chain(ctypes.byref(d), _stream()), "s2m2_mlp_chain")
    _meter("mlp_chain", 2.0 * rows * C * C * (len(stages) + nfan))
    res_t = (out,) + ((normed,) if normed is not None else ()) + ((fan_out,) if fan_out is not None else ())
    return res_t[0] if len(res_t) == 1 else res_t


def conv_block_supported(C: int, H: int, W: int, dtype: torch.dtype) -> bool:
    """K14 (conv_block) takes a ConvBlock2D of this width on an H x W grid (fp16, C = 128 / 256, coarse grids)"""
    return bool(load().s2m2_conv_block_supported(C, H, W, _DT[dtype]))


def conv_block(x: torch.Tensor, w_conv0: torch.Tensor, b_conv0, w_conv2: torch.Tensor, b_conv2, w_1x0: torch.Tensor, b_1x0, w_1x2: torch.Tensor, b_1x2,
               patch_rows: int = 0) -> torch.Tensor:
    """K14: ConvBlock2D (attentions.py:255-281) on x (N,H,W,C) in one launch: convs.2(GELU(convs.0(x))) + convs_1x.2(ReLU(convs_1x.0(x))).
    w_conv0 / w_conv2: the 3x3 layers as K5 v5 fragment streams (pack.pack_conv_frag), w_1x0 / w_1x2: the 1x1 layers in K9's fragment order
    (pack.chain_frag); biases fp32 (C) or None."""
    _resident("conv_block", x, w_conv0, b_conv0, w_conv2, b_conv2, w_1x0, b_1x0, w_1x2, b_1x2)
    if x.dtype != torch.float16:
        raise ValueError("conv_block: x must be an (N,H,W,C) fp16 tensor")
    xs = _pixels(x, "conv_block: x")
    N, H, W, C = x.shape
    d = ConvBlockDesc()
    out = torch.empty((N, H, W, C), device=x.device, dtype=x.dtype)
    d.x, d.x_stride, d.out, d.out_stride, d.N, d.H, d.W, d.C = x.data_ptr(), xs, out.data_ptr(), C, N, H, W, C
    for name, w, n in (("w_conv0", w_conv0, 9 * C * C), ("w_conv2", w_conv2, 9 * C * C), ("w_1x0", w_1x0, C * C), ("w_1x2", w_1x2, C * C)):
        _vec(w, n, f"conv_block: {name}", dtype=x.dtype)
        setattr(d, name, w.data_ptr())
    for name, b in (("b_conv0", b_conv0), ("b_conv2", b_conv2), ("b_1x0", b_1x0), ("b_1x2", b_1x2)):
        _vec(b, C, f"conv_block: {name}", optional=True)
        setattr(d, name, _ptr(b))
    d.patch_rows, d.dtype = patch_rows, _DT[x.dtype]
    _check(load().s2m2_conv_block(ctypes.byref(d), _stream()), "s2m2_conv_block")
    _meter("conv_block", 2.0 * N * H * W * C * C * 20)
    return out


def row_attn_supported(C: int, heads: int, w: int, dtype: torch.dtype) -> bool:
    """K13 (row_attn) exists for rows of w tokens x C channels with this many heads (fp16, C = 128, 1 or 2 heads, w <= 320)"""
    return bool(load().s2m2_row_attn_supported(C, heads, w, _DT[dtype]))


def row_attn(x: torch.Tensor, heads: int, cross: bool, weights: torch.Tensor, vectors: torch.Tensor, ln_eps: float = 1e-5,
             ln_out_eps: Optional[float] = None, xcd_hint: bool = True):
    """K13: one 1-D attention step of BasicAttnBlock (attentions.py:347-355) on the token rows of x (nimg, h, w, 128) in one launch:
    z' = z + proj(attention(LN(z), LN(s)));  out = z' + ffn(LN(z'))  with s = the same line of image (n + nimg/2) % nimg (cross) or z itself.
    weights: (6 * 128, 128) fp16 -- q, k, v, proj, ffn.0, ffn.2 in the row_attn packing (pack.rowattn_pack); vectors: (12, 128) fp32 --
    bias q, row sums q, bias k, row sums k, bias v, row sums v, bias proj, bias ffn.0, row sums ffn.0, bias ffn.2, ln_out gamma, ln_out beta
    (pack.rowattn_vectors).  ln_out_eps: also return LayerNorm(out) * gamma + beta with that eps -> (out, normalised)."""
    _resident("row_attn", x, weights, vectors)
    if x.dtype != torch.float16:
        raise ValueError("row_attn: x must be an (nimg, h, w, C) fp16 tensor")
    xs = _pixels(x, "row_attn: x")
    nimg, h, w, C = x.shape
    _mat(weights, (6 * C, C), x.dtype, "row_attn: weights (pack.rowattn_pack)")
    _mat(vectors, (12, C), torch.float32, "row_attn: vectors (pack.rowattn_vectors)")
    d = RowAttnDesc()
    out = torch.empty((nimg, h, w, C), device=x.device, dtype=x.dtype)
    d.x, d.x_stride, d.out, d.out_stride = x.data_ptr(), xs, out.data_ptr(), C
    d.nimg, d.h, d.w, d.C, d.heads, d.cross, d.ln_eps, d.dtype = nimg, h, w, C, heads, int(bool(cross)), ln_eps, _DT[x.dtype]
    d.xcd_hint = int(bool(xcd_hint))
    d.weights, d.vectors = weights.data_ptr(), vectors.data_ptr()
    normed = None
    if ln_out_eps is not None:
        normed = torch.empty((nimg, h, w, C), device=x.device, dtype=x.dtype)
        d.ln_out, d.ln_out_stride, d.ln_out_eps = normed.data_ptr(), C, float(ln_out_eps)
    rows = nimg * h * w
    flops = 2.0 * rows * C * C * 6 + 4.0 * nimg * h * w * w * C
    with _bracket(ROW_EVENTS, flops, 2.0 * rows * C * (3 if normed is not None else 2),      # unique bytes: rows read once, written once (+ ln_out)
                  f"({nimg},{h},{w},{C}) heads {heads} {'cross' if cross else 'self'}"):
        _check(load().s2m2_row_attn(ctypes.byref(d), _stream()), "s2m2_row_attn")
    _meter("row_attn", flops)
    return out if normed is None else (out, normed)


def pw_direct_supported(K: int, Cout: int, dtype: torch.dtype) -> bool:
    """K11 exists for this layer shape (K = concatenated input channels, multiple of 8)"""
    return bool(load().s2m2_pw_direct_supported(K, Cout, _DT[dtype]))


def pw_direct(srcs, weight_frag: torch.Tensor, bias: Optional[torch.Tensor], Cout: int, act: int = ACT_NONE, shuffle2: int = 0) -> torch.Tensor:
    """K11: a 1x1 layer on the channel concatenation of ``srcs`` ((N,H,W,Ci) / (..., Ci) tensors with contiguous channels and the same leading
    shape), weight in the fragment order of pack.pw_frag, fp32 bias (Cout) or None -> (..., Cout).  shuffle2 = C' > 0: the ConvTranspose2d(2,
    stride 2) store, Cout = 4 * C' -> (N, 2H, 2W, C')."""
    _resident("pw_direct", *srcs, weight_frag, bias)
    x0 = srcs[0]
    d = PwDesc()
    d.nsrc = len(srcs)
    K = 0
    rows = None
    for i, x in enumerate(srcs):
        r, xs = _rows(x, "pw_direct")
        if (rows is not None and r != rows) or x.dtype != x0.dtype:
            raise ValueError("pw_direct: sources must have the same number of rows and one dtype")
        rows = r
        d.src[i], d.src_c[i], d.src_stride[i] = x.data_ptr(), x.shape[-1], xs
        K += x.shape[-1]
    _frag(weight_frag, Cout, K, x0.dtype, "pw_direct: weight (pack.pw_frag)")
    _vec(bias, Cout, "pw_direct: bias", at_least=True, optional=True)
    if shuffle2:
        if x0.dim() != 4 or Cout != 4 * shuffle2:
            raise ValueError("pw_direct: shuffle2 needs (N,H,W,C) sources and Cout = 4 * shuffle2")
        out = torch.empty((x0.shape[0], 2 * x0.shape[1], 2 * x0.shape[2], shuffle2), device=x0.device, dtype=x0.dtype)
        d.shuffle2, d.Ho, d.Wo, d.out_stride = shuffle2, x0.shape[1], x0.shape[2], shuffle2
    else:
        out = torch.empty(tuple(x0.shape[:-1]) + (Cout,), device=x0.device, dtype=x0.dtype)
        d.out_stride = Cout
    d.rows, d.weight_frag, d.bias, d.out = rows, weight_frag.data_ptr(), _ptr(bias), out.data_ptr()
    d.Cout, d.act, d.dtype = Cout, act, _DT[x0.dtype]
    _check(load().s2m2_pw_direct(ctypes.byref(d), _stream()), "s2m2_pw_direct")
    _meter("conv2d", 2.0 * rows * K * Cout)                          # (as K5 counts the same layer: no MFMA-tile padding)
    return out


def conv_narrow_supported(KH: int, KW: int, stride: int, Cin: int, Cout: int, dtype: torch.dtype) -> bool:
    """K12 exists for this layer shape (Cin = ALL input channels of the one or two sources)"""
    return bool(load().s2m2_conv_narrow_supported(KH, KW, stride, Cin, Cout, _DT[dtype]))


def conv_narrow(srcs, weight_frag: torch.Tensor, bias: Optional[torch.Tensor], KH: int, KW: int, Cout: int, stride: int = 1,
                act: int = ACT_NONE, head=None) -> torch.Tensor:
    """K12: a KH x KW convolution (padding K // 2) in the pixel-split direct form on one (N,H,W,Cin) tensor -- or the channel concatenation
    of two -- weight = pack.narrow_frag of the K-order-0 matrix (Cout, KH*KW*Cin), fp32 bias (Cout) or None
    -> (N, ceil(H/stride), ceil(W/stride), Cout).  Shapes: conv_narrow_supported.
    head = (pack.head_frag of a (Cout2, Cout) 1x1 weight, fp32 bias (Cout2) or None, Cout2): that 1x1 layer applied to the activated output
    inside the same launch (Cin = 48 form) -> (..., Cout2); the Cout-channel tensor is not produced."""
    if isinstance(srcs, torch.Tensor):
        srcs = [srcs]
    hf, hb, cout_final = head if head is not None else (None, None, Cout)
    _resident("conv_narrow", *srcs, weight_frag, bias, hf, hb)
    if not 1 <= len(srcs) <= 2 or any(t.shape[:3] != srcs[0].shape[:3] or t.dtype != srcs[0].dtype for t in srcs):
        raise ValueError("conv_narrow: one or two (N,H,W,C) sources of the same grid and dtype")
    x = srcs[0]
    xs = _pixels(x, "conv_narrow: source")
    n, h, w, _ = x.shape
    cin = sum(t.shape[-1] for t in srcs)
    K = KH * KW * cin
    _frag(weight_frag, Cout, K, x.dtype, "conv_narrow: weight (pack.narrow_frag)")
    _vec(bias, Cout, "conv_narrow: bias", at_least=True, optional=True)
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    if head is not None:
        _mat(hf, (1, 2 * ((Cout + 31) // 32), 64, 8), x.dtype, f"conv_narrow: head weight (pack.head_frag of a (Cout2, {Cout}) matrix)")
        _vec(hb, cout_final, "conv_narrow: head bias", at_least=True, optional=True)
    out = torch.empty((n, ho, wo, cout_final), device=x.device, dtype=x.dtype)
    d = NarrowDesc()
    if head is not None:
        d.head_frag, d.head_bias, d.head_cout = hf.data_ptr(), _ptr(hb), cout_final
    d.x, d.x_stride, d.N, d.H, d.W, d.Cin = x.data_ptr(), xs, n, h, w, cin
    if len(srcs) == 2:
        d.x1, d.x1_stride, d.Cin1 = srcs[1].data_ptr(), _pixels(srcs[1], "conv_narrow: source"), srcs[1].shape[-1]
    d.weight_frag, d.bias, d.out, d.out_stride = weight_frag.data_ptr(), _ptr(bias), out.data_ptr(), cout_final
    d.Cout, d.KH, d.KW, d.stride, d.act, d.dtype = Cout, KH, KW, stride, act, _DT[x.dtype]
    _check(load().s2m2_conv_narrow(ctypes.byref(d), _stream()), "s2m2_conv_narrow")
    _meter("conv2d", 2.0 * n * ho * wo * (K * Cout + (Cout * cout_final if head is not None else 0)))   # (as K5 counts the same layers: no MFMA-tile padding)
    return out


def feature_fusion_supported(C: int, dtype: torch.dtype) -> bool:
    return bool(load().s2m2_feature_fusion_supported(C, _DT[dtype]))


def feature_fusion_frag_supported(C: int, dtype: torch.dtype) -> bool:
    """the direct form of K10 (weights as a fragment stream, pack.fusion_frag) exists for this width"""
    return bool(load().s2m2_feature_fusion_frag_supported(C, _DT[dtype]))


def feature_fusion(z0: torch.Tensor, z1: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: Optional[torch.Tensor], bg: torch.Tensor,
                   bf: torch.Tensor, z1_coarse: bool = False, frag: bool = False) -> torch.Tensor:
    """FeatureFusion with 1x1 kernels in one launch (s2m2_feature_fusion): z0, z1 (..., C); w1 packed (3C, 2C) = [gate.0; fusion.0],
    w2 packed (C, 3C) = [gate.2 | fusion.2]; biases fp32.  z1_coarse: z0 is (N, 2h, 2w, C) and z1 the coarse (N, h, w, C) tensor,
    read through the bilinear x2 resampling.  frag: w1 is the fragment stream of BOTH layers (pack.fusion_frag(w1, w2), 9*C*C values),
    w2 is None -> the direct form (s2m2_feature_fusion_frag), meant for short row counts."""
    _resident("feature_fusion", z0, z1, w1, b1, w2, bg, bf)
    C = z0.shape[-1]
    if z1.dtype != z0.dtype or z1.shape[-1] != C:
        raise ValueError("feature_fusion: z0 and z1 must match")
    hc = wc = 0
    if z1_coarse:
        if z0.dim() != 4 or z1.dim() != 4 or tuple(z0.shape[:3]) != (z1.shape[0], 2 * z1.shape[1], 2 * z1.shape[2]):
            raise ValueError("feature_fusion: z1_coarse needs z0 (N,2h,2w,C) and z1 (N,h,w,C)")
        hc, wc = z1.shape[1], z1.shape[2]
    elif z1.shape != z0.shape:
        raise ValueError("feature_fusion: z0 and z1 must match")
    if frag:
        if w2 is not None:
            raise ValueError("feature_fusion: frag takes the fragment stream of both layers as w1 and w2 = None")
        _vec(w1, 9 * C * C, "feature_fusion: w1 (pack.fusion_frag)", dtype=z0.dtype)
    else:
        _mat(w1, (3 * C, 2 * C), z0.dtype, "feature_fusion: w1")
        _mat(w2, (C, 3 * C), z0.dtype, "feature_fusion: w2")
    for name, t, n in (("b1", b1, 3 * C), ("bg", bg, C), ("bf", bf, C)):
        _vec(t, n, f"feature_fusion: bias {name}")
    rows, s0 = _rows(z0, "feature_fusion: z0")
    _, s1 = _rows(z1, "feature_fusion: z1")
    out = torch.empty(z0.shape, device=z0.device, dtype=z0.dtype)
    head = (z0.data_ptr(), z1.data_ptr(), out.data_ptr(), s0, s1, C, rows, C, w1.data_ptr(), b1.data_ptr())
    tail = (bg.data_ptr(), bf.data_ptr(), hc, wc, _DT[z0.dtype], _stream())
    if frag:                                                        # the direct form takes no second weight
        _check(load().s2m2_feature_fusion_frag(*head, *tail), "s2m2_feature_fusion_frag")
    else:
        _check(load().s2m2_feature_fusion(*head, w2.data_ptr(), *tail), "s2m2_feature_fusion")
    _meter("feature_fusion", 2.0 * rows * C * C * 9)                # (2C -> 3C) + (C -> C) + (2C -> C)
    return out


def layernorm(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm without affine over the last axis of a (..., C) tensor with contiguous channels and a uniform row stride."""
    _resident("layernorm", x, out)
    C = x.shape[-1]
    rows, xs = _rows(x, "layernorm")
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    else:
        _mat(out, x.shape, x.dtype, "layernorm: out")
    _check(load().s2m2_layernorm(x.data_ptr(), out.data_ptr(), rows, C, xs, C, _DT[x.dtype], _stream()), "s2m2_layernorm")
    return out


def groupnorm_nhwc(x: torch.Tensor, groups: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """nn.GroupNorm on a contiguous (N,H,W,C) tensor; gamma/beta fp32."""
    _resident("groupnorm_nhwc", x, gamma, beta)
    _contig("groupnorm_nhwc", x, gamma, beta)
    n, h, w, c = x.shape
    ws = torch.empty(load().s2m2_groupnorm_workspace_bytes(n, groups) // 8, device=x.device, dtype=torch.float64)
    out = torch.empty_like(x)
    _check(load().s2m2_groupnorm_nhwc(x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ws.data_ptr(), n, h * w, c,
                                      groups, eps, _DT[x.dtype], _stream()), "s2m2_groupnorm_nhwc")
    return out


def convex_upsample(maps, logits: torch.Tensor, factor: int, scales=None, logit_up2: bool = False,
                    chan_out: Optional[torch.Tensor] = None):
    """maps: list of (B,1,hs,ws) or (B,hs,ws) fp32 tensors; logits (B,Ho,Wo,>=16) NHWC (9 used).  -> list of (B,1,Ho,Wo) fp32.
    chan_out: optional (B,Ho,Wo) view (one channel of an NHWC tensor, dense pixels) that also receives map 0 in its dtype."""
    _resident("convex_upsample", *maps, logits, chan_out)
    B, hs, ws = maps[0].shape[0], maps[0].shape[-2], maps[0].shape[-1]
    n = len(maps)
    maps = [m.float().contiguous() for m in maps]
    ls = _pixels(logits, "convex_upsample: logits")
    Ho, Wo = hs * factor, ws * factor
    exp_l = (B, hs, ws) if logit_up2 else (B, Ho, Wo)
    if tuple(logits.shape[:3]) != exp_l:
        raise ValueError(f"convex_upsample: logits must be {exp_l + ('>=16',)}, got {tuple(logits.shape)}")
    base = torch.empty((n, B, 1, Ho, Wo), device=logits.device, dtype=torch.float32)      # one allocation: callers can copy all maps at once
    outs = [base[k] for k in range(n)]
    sc = (ctypes.c_float * n)(*[float(v) for v in (scales or [1.0] * n)])
    cs = 0
    if chan_out is not None:
        if chan_out.dtype != logits.dtype or tuple(chan_out.shape) != (B, Ho, Wo):
            raise ValueError("convex_upsample: chan_out must be a (B,Ho,Wo) channel view in the logits dtype")
        cs = _pixels(chan_out.unsqueeze(-1), "convex_upsample: chan_out")       # as (B,Ho,Wo,1): the pixels of a one-channel NHWC view
    _check(load().s2m2_convex_upsample(_ptrs(maps), _ptrs(outs), sc, n, logits.data_ptr(), ls, B, hs, ws, factor, int(logit_up2),
                                       _ptr(chan_out), cs, _DT[logits.dtype], _stream()), "s2m2_convex_upsample")
    return outs


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, swap_halves: bool = False,
              pe: Optional[Tuple[torch.Tensor, torch.Tensor, int, int]] = None, scale: Optional[float] = None):
    """q, k, v: (nb, N, heads*D) views with contiguous channels and dense token rows (e.g. slices of a fused QKV buffer).
    -> out (nb, Nq, heads*D) [, pe_sum (nb, Nq, heads*32) when pe = (px (2w-1,16) fp32, py (2h-1,16) fp32, w, h)]."""
    px, py, gw, gh = pe if pe is not None else (None, None, 0, 0)
    _resident("attention", q, k, v, px, py)
    _contig("attention: pe tables", px, py)
    nb, Nq, C = q.shape
    Nk = k.shape[1]
    D = C // heads
    qs, ks, vs = (_rows(t, f"attention: {name}")[1] for name, t in (("q", q), ("k", k), ("v", v)))
    out = torch.empty((nb, Nq, C), device=q.device, dtype=q.dtype)
    pe_out = torch.empty((nb, Nq, heads * 32), device=q.device, dtype=q.dtype) if pe is not None else None
    flops = 4.0 * nb * heads * Nq * Nk * D                            # QK^T + PV (4 N^2 d per batch x head)
    with _bracket(ATTN_EVENTS, flops, f"({nb},{heads},{Nq},{D}){'+pe' if pe is not None else ''}",
                  2.0 * nb * heads * D * (2 * Nq + 2 * Nk)):          # unique bytes: q, k, v read + o written (fp16)
        _check(load().s2m2_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), qs, ks, vs, C, nb, heads, Nq, Nk, D,
                                     float(scale if scale is not None else D ** -0.5), int(swap_halves), _ptr(px), _ptr(py), _ptr(pe_out),
                                     heads * 32, gw, gh, _DT[q.dtype], _stream()), "s2m2_attention")
    _meter("attention", flops)
    return (out, pe_out) if pe is not None else out


def attention_supported(nb: int, heads: int, N: int, D: int, dtype: torch.dtype, grid: Optional[Tuple[int, int]] = None) -> Tuple[bool, str]:
    """Would s2m2_attention take this launch?  grid = (w, h) of the token grid for the PE variant.  -> (ok, reason)."""
    gw, gh = grid if grid is not None else (0, 0)
    lib = load()
    ok = bool(lib.s2m2_attention_supported(nb, heads, N, D, gw, gh, _DT[dtype]))
    return ok, ("" if ok else lib.s2m2_last_error().decode())


def attention_plan(nb: int, heads: int, Nq: int, Nk: int, D: int, dtype: torch.dtype, swap_halves: bool = False,
                   grid: Optional[Tuple[int, int]] = None) -> dict:
    """The launch s2m2_attention would make, from its own planner (s2m2_attention_plan; host code, no device needed) -> the fields of
    s2m2_attn_plan by name.  Raises with the planner's message where it refuses the call."""
    gw, gh = grid if grid is not None else (0, 0)
    p = AttnPlan()
    _check(load().s2m2_attention_plan(nb, heads, Nq, Nk, D, int(swap_halves), gw, gh, _DT[dtype], ctypes.byref(p)), "s2m2_attention_plan")
    return {n: int(getattr(p, n)) for n, _ in AttnPlan._fields_}


def resample2x(x: torch.Tensor, mode: int) -> torch.Tensor:
    """(N,H,W,C) -> AvgPool2d(2) (mode 0) or bilinear x2, align_corners=False (mode 1)."""
    _resident("resample2x", x)
    xs = _pixels(x, "resample2x")
    n, h, w, c = x.shape
    out = torch.empty((n, h // 2, w // 2, c) if mode == 0 else (n, 2 * h, 2 * w, c), device=x.device, dtype=x.dtype)
    _check(load().s2m2_resample2x(x.data_ptr(), out.data_ptr(), n, h, w, c, xs, c, mode, _DT[x.dtype], _stream()), "s2m2_resample2x")
    return out


def cv_lookup_into(cv: torch.Tensor, disp: torch.Tensor, buf: torch.Tensor, off1: int, off2: int, radius: int = 4) -> None:
    """K3 writing straight into channel slots of a wider NHWC tensor: taps of level 0 -> buf[..., off1:off1+2r+1], level 1 ->
    buf[..., off2:off2+2r+1] (buf (B,h,w,Cb) contiguous, fp16 or fp32; the other channels are left untouched; the two ranges lie inside
    a pixel's Cb channels and apart from each other: _lookup_geometry)."""
    _resident("cv_lookup_into", cv, disp, buf)
    pitch = _lookup_geometry("cv_lookup_into", cv, disp, radius, buf, off1, off2)
    B, h, w, _ = cv.shape
    cb = buf.shape[-1]
    es = buf.element_size()
    _check(load().s2m2_cv_lookup(cv.data_ptr(), disp.data_ptr(), buf.data_ptr() + off1 * es, buf.data_ptr() + off2 * es, B, h, w,
                                 radius, _DT[cv.dtype], _DT[buf.dtype], h * w * cb, cb, 1, pitch, _stream()), "s2m2_cv_lookup")


_IMG_DT = {torch.float32: 0, torch.float16: 1, torch.uint8: 2}


def image_prep(img0: torch.Tensor, img1: torch.Tensor, dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """img0, img1 (B,3,H,W) fp32 / fp16 / uint8 in [0,255] -> x8 (2B,H,W,8): channels 1..3 = normalised RGB, others 0 (``out``: written in place)."""
    _resident("image_prep", img0, img1, out)
    if img0.dtype not in _IMG_DT:
        img0 = img0.float()
    img1 = img1.to(img0.dtype)
    img0, img1 = img0.contiguous(), img1.contiguous()
    B, _, H, W = img0.shape
    if out is not None:
        _mat(out, (2 * B, H, W, 8), dtype, "image_prep: out")
        x8 = out
    else:
        x8 = torch.empty((2 * B, H, W, 8), device=img0.device, dtype=dtype)
    _check(load().s2m2_image_prep(img0.data_ptr(), img1.data_ptr(), x8.data_ptr(), B, H, W, _IMG_DT[img0.dtype], _DT[dtype], _stream()),
           "s2m2_image_prep")
    return x8


def clock_probe(out: torch.Tensor) -> None:
    """Measurement aid: out (2,) int64 device tensor <- {shader-clock ticks, 100 MHz real-time ticks} when the stream reaches this point."""
    _resident("clock_probe", out)
    _contig("clock_probe", out)
    _check(load().s2m2_debug_clock_probe(out.data_ptr(), _stream()), "s2m2_debug_clock_probe")


def poison_lds() -> None:
    """Test aid: quiet-NaN patterns in the LDS of every CU (s2m2_debug_poison_lds), on the current stream."""
    _check(load().s2m2_debug_poison_lds(_stream()), "s2m2_debug_poison_lds")


def refine_prep(disp: torch.Tensor, conf: torch.Tensor, occ: Optional[torch.Tensor], mode: int, dtype: torch.dtype) -> torch.Tensor:
    """(B,1,h,w) fp32 maps -> (B,h,w,8) side input of the global (mode 0) / local (mode 1) refiner."""
    _resident("refine_prep", disp, conf, occ)
    _contig("refine_prep", disp, conf, occ)
    B, _, h, w = disp.shape
    out = torch.empty((B, h, w, 8), device=disp.device, dtype=dtype)
    _check(load().s2m2_refine_prep(disp.data_ptr(), conf.data_ptr(), _ptr(occ), out.data_ptr(), B * h * w, mode, _DT[dtype], _stream()),
           "s2m2_refine_prep")
    return out


def global_update(upd: torch.Tensor, disp: torch.Tensor, conf: torch.Tensor, clamp0: bool) -> torch.Tensor:
    """upd (B,h,w,C>=1) NHWC (channel 0 used), disp/conf (B,1,h,w) fp32 -> refined disparity (B,1,h,w) fp32."""
    _resident("global_update", upd, disp, conf)
    _contig("global_update", disp, conf)
    out = torch.empty_like(disp)
    _check(load().s2m2_global_update(upd.data_ptr(), _pixels(upd, "global_update: upd"), disp.data_ptr(), conf.data_ptr(), out.data_ptr(),
                                     disp.numel(), int(clamp0), _DT[upd.dtype], _stream()), "s2m2_global_update")
    return out


def refine_update(dco: torch.Tensor, disp: torch.Tensor, conf: torch.Tensor, occ: torch.Tensor, use_positivity: bool,
                  want_small: bool = False):
    """dco (B,h,w,>=10) NHWC deltas; disp/conf/occ (B,1,h,w) fp32 -> new (disp, conf, occ) (fresh tensors) [, small (B,h,w,8): the
    refine_prep(mode 1) side input of the next iteration, from the same launch]."""
    _resident("refine_update", dco, disp, conf, occ)
    _contig("refine_update", disp, conf, occ)
    outs = torch.empty((3,) + tuple(disp.shape), device=disp.device, dtype=torch.float32)
    small = torch.empty((disp.shape[0], disp.shape[-2], disp.shape[-1], 8), device=disp.device, dtype=dco.dtype) if want_small else None
    _check(load().s2m2_refine_update_to(dco.data_ptr(), _pixels(dco, "refine_update: dco"), disp.data_ptr(), conf.data_ptr(), occ.data_ptr(),
                                        outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), _ptr(small), disp.numel(), disp.shape[-1],
                                        int(use_positivity), _DT[dco.dtype], _stream()), "s2m2_refine_update_to")
    return (outs[0], outs[1], outs[2], small) if want_small else (outs[0], outs[1], outs[2])


def tanh(x: torch.Tensor) -> torch.Tensor:
    _resident("tanh", x)
    _contig("tanh", x)
    y = torch.empty_like(x)
    _check(load().s2m2_tanh(x.data_ptr(), y.data_ptr(), x.numel(), _DT[x.dtype], _stream()), "s2m2_tanh")
    return y


def stem_mlp(x8: torch.Tensor, w0: torch.Tensor, b0: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor) -> torch.Tensor:
    """(N,H,W,8) -> (N,H,W,16): Conv1x1(8->16) - GELU - Conv1x1(16->16) per pixel (s2m2_stem_mlp); fp32 weights (16,8), (16,16), biases (16)."""
    _resident("stem_mlp", x8, w0, b0, w1, b1)
    _contig("stem_mlp", x8)
    if x8.shape[-1] != 8:
        raise ValueError("stem_mlp: x8 must be (..., 8)")
    _mat(w0, (16, 8), torch.float32, "stem_mlp: w0")
    _mat(w1, (16, 16), torch.float32, "stem_mlp: w1")
    _vec(b0, 16, "stem_mlp: b0")
    _vec(b1, 16, "stem_mlp: b1")
    out = torch.empty(tuple(x8.shape[:-1]) + (16,), device=x8.device, dtype=x8.dtype)
    _check(load().s2m2_stem_mlp(x8.data_ptr(), w0.data_ptr(), b0.data_ptr(), w1.data_ptr(), b1.data_ptr(), out.data_ptr(),
                                x8.numel() // 8, _DT[x8.dtype], _stream()), "s2m2_stem_mlp")
    return out


def image_pad(img: torch.Tensor, factor: int = 32) -> torch.Tensor:
    """Reference image_pad (image_utils.py:27-71) on the device: (B,C,H,W) fp32/fp16/uint8 -> (B,C,Hn,Wn) fp32."""
    _resident("image_pad", img)
    if img.dtype not in _IMG_DT:
        img = img.float()
    img = img.contiguous()
    B, C, H, W = img.shape
    Hn, Wn = -(-H // factor) * factor, -(-W // factor) * factor
    pooled = torch.empty((B, C, H // factor, W // factor), device=img.device, dtype=torch.float32)
    out = torch.empty((B, C, Hn, Wn), device=img.device, dtype=torch.float32)
    _check(load().s2m2_image_pad(img.data_ptr(), pooled.data_ptr(), out.data_ptr(), B, C, H, W, factor, _IMG_DT[img.dtype], _stream()),
           "s2m2_image_pad")
    return out


def _opt(t: Optional[torch.Tensor], shape, dtype: torch.dtype, what: str):
    """an optional output: None -> NULL; a contiguous tensor of exactly this shape and dtype (_mat) -> its pointer"""
    if t is None:
        return None
    _mat(t, shape, dtype, what)
    return t.data_ptr()


def _extent_query(symbol: str, stage: str, **extents: int) -> int:
    """the extent queries of the output stages (workspace bytes, tile rows / columns): the library answers 0 for extents it refuses"""
    n = int(getattr(load(), symbol)(*extents.values()))
    if n == 0:
        raise ValueError(f"{stage}: bad extents " + " ".join(f"{k}={v}" for k, v in extents.items()))
    return n


def _cloud_inputs(what: str, d: CloudDesc, disp, occ, conf, image, H, W, fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min,
                  occ_min, unfiltered) -> Tuple[int, int, int]:
    """the input half of ``d``, which s2m2_cloud, s2m2_mesh, s2m2_register and s2m2_segment all take: the three maps, the image (or, with
    ``image`` None, the extents ``H`` x ``W`` of the fused crop), the camera and filter numbers -> (B, H, W)"""
    if disp.dtype != torch.float32 or occ.dtype != torch.float32 or conf.dtype != torch.float32 or disp.dim() != 4 or disp.shape[1] != 1:
        raise ValueError(f"{what}: disp / occ / conf must be (B,1,Hp,Wp) fp32 tensors")
    if occ.shape != disp.shape or conf.shape != disp.shape:
        raise ValueError(f"{what}: disp, occ and conf must have one shape")
    B, _, Hp, Wp = disp.shape
    if image is not None:
        if image.dtype not in _IMG_DT or image.dim() != 4 or image.shape[1] != 3 or image.shape[0] != B:
            raise ValueError(f"{what}: image must be a (B,3,H,W) uint8 / fp16 / fp32 tensor")
        if (H is not None and H != image.shape[2]) or (W is not None and W != image.shape[3]):
            raise ValueError(f"{what}: H and W differ from the image")
        H, W = image.shape[-2:]
        d.image, d.image_dtype = image.data_ptr(), _IMG_DT[image.dtype]
    elif H is None or W is None:
        raise ValueError(f"{what}: without an image, H and W are required")
    else:
        d.image_dtype = _IMG_DT[torch.uint8]
    d.disp, d.occ, d.conf = disp.data_ptr(), occ.data_ptr(), conf.data_ptr()
    d.B, d.H, d.W, d.Hp, d.Wp, d.unfiltered = B, H, W, Hp, Wp, int(unfiltered)
    d.fx, d.fy, d.cx, d.cy, d.baseline, d.doffs = fx, fy, cx, cy, baseline, doffs
    d.depth_scale, d.depth_trunc, d.conf_min, d.occ_min = depth_scale, depth_trunc, conf_min, occ_min
    return B, H, W


def _cloud_outputs(what: str, d: CloudDesc, need, records, count, workspace, depth, mask) -> None:
    """K15's outputs in ``d`` (s2m2_cloud, s2m2_mesh), behind _cloud_inputs; ``need(B, H, W)``: the workspace bytes that ``count`` requires"""
    B, H, W = d.B, d.H, d.W
    d.depth = _opt(depth, (B, 1, H, W), torch.float32, f"{what}: depth")
    d.mask = _opt(mask, (B, 1, H, W), torch.uint8, f"{what}: mask")
    if count is not None:
        _vec(count, B, f"{what}: count", dtype=torch.int32)
        need = need(B, H, W)
        if workspace is None or workspace.nbytes < need:
            raise ValueError(f"{what}: a workspace of {need} bytes is required with count")
        d.count, d.workspace = count.data_ptr(), workspace.data_ptr()
        if records is not None:
            if records.dtype != torch.int32 or records.dim() != 3 or records.shape[0] != B or records.shape[2] != 4:
                raise ValueError(f"{what}: records must be a (B, capacity, 4) int32 tensor")
            d.capacity = records.shape[1]
            d.records = records.data_ptr() if records.shape[1] > 0 else None
    elif records is not None:
        raise ValueError(f"{what}: records come with count")


def cloud(disp: torch.Tensor, occ: torch.Tensor, conf: torch.Tensor, image: torch.Tensor, *, fx: float, fy: float, cx: float, cy: float,
          baseline: float, doffs: float = 0.0, depth_scale: float = 1000.0, depth_trunc: float = 0.0, conf_min: float = 0.1,
          occ_min: float = 0.5, unfiltered: bool = False, records: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
          workspace: Optional[torch.Tensor] = None, depth: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> None:
    """s2m2_cloud (K15): the padded maps (B,1,Hp,Wp) fp32 and the UNPADDED left image (B,3,H,W) uint8 / fp16 / fp32 -> the outputs the caller
    allocated: ``records`` (B, capacity, 4) int32 = 16-byte point records in raster order with ``count`` (B) int32 and a ``workspace`` of
    ``cloud_workspace_bytes`` bytes, ``depth`` (B,1,H,W) fp32, ``mask`` (B,1,H,W) uint8.  Thin: no allocation, no synchronisation."""
    _resident("cloud", disp, occ, conf, image, records, count, workspace, depth, mask)
    _contig("cloud", disp, occ, conf, image, records, count, workspace, depth, mask)
    d = CloudDesc()
    _cloud_inputs("cloud", d, disp, occ, conf, image, None, None, fx, fy, cx, cy, baseline, doffs, depth_scale, depth_trunc, conf_min, occ_min, unfiltered)
    _cloud_outputs("cloud", d, cloud_workspace_bytes, records, count, workspace, depth, mask)
    with torch.cuda.device(disp.device):
        _check(load().s2m2_cloud(ctypes.byref(d), _stream()), "s2m2_cloud")


def cloud_workspace_bytes(B: int, H: int, W: int) -> int:
    return _extent_query("s2m2_cloud_workspace_bytes", "cloud", B=B, H=H, W=W)


def rectify(srcs, records: torch.Tensor, out: Optional[torch.Tensor] = None, maps: Optional[torch.Tensor] = None, *, hd: Optional[int] = None,
            wd: Optional[int] = None, round: bool = True, order: int = RECTIFY_ORDER_SAMPLE) -> None:
    """s2m2_rectify (K16): ``srcs`` = one or two raw images of one shape and dtype -- (H,W,3) uint8 interleaved, (3,H,W) uint8 or (3,H,W) fp32 --
    and ``records`` (n_img, RECTIFY_RECORD_FLOATS) fp32 -> the outputs the caller allocated: ``out`` (n_img,3,Hd,Wd) fp32 / uint8 and / or
    ``maps`` (n_img,2,Hd,Wd) fp32.  With ``out`` None no source is read (``srcs`` gives the source extents only; pass ``hd`` / ``wd`` then, or
    they are taken from ``maps``).  Thin: no allocation, no synchronisation."""
    srcs = list(srcs)
    _resident("rectify", *srcs, records, out, maps)
    _contig("rectify", *srcs, records, out, maps)
    if len(srcs) not in (1, 2) or any(t.shape != srcs[0].shape or t.dtype != srcs[0].dtype for t in srcs):
        raise ValueError("rectify: one or two source images of one shape and dtype")
    s0 = srcs[0]
    if s0.dim() == 3 and s0.dtype == torch.uint8 and s0.shape[2] == 3:
        fmt, (Hs, Ws) = RECTIFY_SRC_U8_HWC, s0.shape[:2]
    elif s0.dim() == 3 and s0.shape[0] == 3 and s0.dtype in (torch.uint8, torch.float32):
        fmt, (Hs, Ws) = RECTIFY_SRC_U8_CHW if s0.dtype == torch.uint8 else RECTIFY_SRC_F32_CHW, s0.shape[1:]
    else:
        raise ValueError("rectify: a source is an (H,W,3) uint8, (3,H,W) uint8 or (3,H,W) fp32 tensor")
    if records.dtype != torch.float32 or records.dim() != 2 or records.shape[1] != RECTIFY_RECORD_FLOATS or records.shape[0] < 1:
        raise ValueError(f"rectify: records must be an (n_img, {RECTIFY_RECORD_FLOATS}) fp32 tensor")
    n = records.shape[0]
    if out is None and maps is None:
        raise ValueError("rectify: no output requested")
    ref = out if out is not None else maps
    if ref.dim() != 4:
        raise ValueError("rectify: out is (n_img,3,Hd,Wd), maps is (n_img,2,Hd,Wd)")
    Hd, Wd = (hd, wd) if hd is not None and wd is not None else ref.shape[-2:]
    d = RectifyDesc()
    if out is not None:
        if out.dtype not in (torch.float32, torch.uint8):
            raise ValueError("rectify: out must be an (n_img,3,Hd,Wd) fp32 or uint8 tensor")
        _mat(out, (n, 3, Hd, Wd), out.dtype, "rectify: out")
        d.out, d.out_dtype = out.data_ptr(), _IMG_DT[out.dtype]
        d.src[0], d.src[1] = srcs[0].data_ptr(), srcs[-1].data_ptr()
    d.maps = _opt(maps, (n, 2, Hd, Wd), torch.float32, "rectify: maps")
    d.records, d.n_src, d.n_img, d.Hs, d.Ws, d.Hd, d.Wd = records.data_ptr(), len(srcs), n, Hs, Ws, Hd, Wd
    d.src_format, d.round, d.order = fmt, int(bool(round)), order
    with torch.cuda.device(records.device):
        _check(load().s2m2_rectify(ctypes.byref(d), _stream()), "s2m2_rectify")


# K17 (s2m2_conv_gru): its wrapper lives in hip_gru.py and is re-exported here, so callers write hip.conv_gru like every other launch
from .hip_gru import conv_gru, conv_gru_supported  # noqa: E402,F401
# K18 (s2m2_disp_eval): likewise in hip_eval.py
from .hip_eval import disp_eval, eval_tile_rows, eval_workspace_bytes  # noqa: E402,F401

# K19 (s2m2_conv_block_tail): likewise, from hip_tail.py
from .hip_tail import conv_block_tail, conv_block_tail_supported  # noqa: E402,F401

# K20 (s2m2_mesh): likewise, from hip_mesh.py
from .hip_mesh import mesh, mesh_tile_rows, mesh_workspace_bytes  # noqa: E402,F401

# K21 (s2m2_register): likewise, from hip_register.py
from .hip_register import register, register_workspace_bytes  # noqa: E402,F401
# K22 (s2m2_segment): likewise, from hip_segment.py
from .hip_segment import segment, segment_tile, segment_workspace_bytes  # noqa: E402,F401
# K23 (s2m2_voxel): likewise, from hip_voxel.py
from .hip_voxel import voxel, voxel_home_slot, voxel_slots, voxel_tile_rows, voxel_workspace_bytes  # noqa: E402,F401
# K24 (s2m2_tsdf_integrate, s2m2_tsdf_extract), K25 (s2m2_tsdf_mesh), K26 (s2m2_tsdf_raycast) and K27 (s2m2_tsdf_track): likewise, from
# hip_tsdf.py
from .hip_tsdf import (RAYCAST_MAX_STEPS, TRACK_MAX_ITERS, tsdf_extract, tsdf_integrate, tsdf_mesh, tsdf_mesh_workspace_bytes, tsdf_raycast,  # noqa: E402,F401
                       tsdf_raycast_steps, tsdf_tile_voxels, tsdf_track, tsdf_track_workspace_bytes, tsdf_workspace_bytes)
# K28 (s2m2_normals): likewise, from hip_normals.py
from .hip_normals import NORMALS_MAX_RADIUS, normals  # noqa: E402,F401
# K29 (s2m2_smooth): likewise, from hip_smooth.py
from .hip_smooth import smooth, smooth_weights  # noqa: E402,F401
