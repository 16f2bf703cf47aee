"""K18 (``s2m2_disp_eval``, csrc/evalstats.hip): disparity error statistics against ground truth.  The descriptor mirror, the layout constants
and the signatures are in hip.py with all the others (``hip.load()`` binds every symbol there); this module holds the wrappers, which hip.py
re-exports as ``hip.disp_eval``, ``hip.eval_workspace_bytes`` and ``hip.eval_tile_rows``."""
import ctypes
from typing import Optional

import torch

from . import hip as _h


def eval_workspace_bytes(B: int, H: int, W: int) -> int:
    return _h._extent_query("s2m2_eval_workspace_bytes", "disp_eval", B=B, H=H, W=W)


def eval_tile_rows(H: int, W: int) -> int:
    """image rows of one tile of K18's first launch (a pair of H rows is ceil(H / rows) partial blocks in the workspace)"""
    return _h._extent_query("s2m2_eval_tile_rows", "disp_eval", H=H, W=W)


def disp_eval(disp: torch.Tensor, gt: torch.Tensor, stats: torch.Tensor, workspace: torch.Tensor, *, region: Optional[torch.Tensor] = None,
              occ: Optional[torch.Tensor] = None, conf: Optional[torch.Tensor] = None, thresholds=(0.5, 1.0, 2.0, 4.0), d1_abs: float = 3.0,
              d1_rel: float = 0.05, gt_min: float = 0.0, conf_min: float = 0.1, occ_min: float = 0.5) -> None:
    """s2m2_disp_eval (K18): the padded maps (B,1,Hp,Wp) fp32 (occ and conf together or not at all), the UNPADDED ground truth (B,1,H,W) fp32 and
    the optional region mask (B,1,H,W) uint8 -> ``stats`` (B, hip.EVAL_WORDS) int64, every word written; ``workspace``: ``eval_workspace_bytes``
    bytes.  Thin: no allocation, no synchronisation."""
    _h._resident("disp_eval", disp, gt, stats, workspace, region, occ, conf)
    _h._contig("disp_eval", disp, workspace)
    if disp.dtype != torch.float32 or disp.dim() != 4 or disp.shape[1] != 1 or gt.dim() != 4:
        raise ValueError("disp_eval: disp must be a (B,1,Hp,Wp) fp32 tensor and gt a (B,1,H,W) fp32 tensor")
    if (occ is None) != (conf is None):
        raise ValueError("disp_eval: occ and conf come together")
    B, _, Hp, Wp = disp.shape
    H, W = gt.shape[-2:]
    _h._mat(gt, (B, 1, H, W), torch.float32, "disp_eval: gt")
    _h._mat(stats, (B, _h.EVAL_WORDS), torch.int64, "disp_eval: stats")
    d = _h.EvalDesc()
    d.occ = _h._opt(occ, (B, 1, Hp, Wp), torch.float32, "disp_eval: occ")
    d.conf = _h._opt(conf, (B, 1, Hp, Wp), torch.float32, "disp_eval: conf")
    d.region = _h._opt(region, (B, 1, H, W), torch.uint8, "disp_eval: region")
    thresholds = tuple(float(t) for t in thresholds)
    if len(thresholds) > _h.EVAL_MAX_THR:
        raise ValueError(f"disp_eval: at most {_h.EVAL_MAX_THR} thresholds, got {len(thresholds)}")
    need = eval_workspace_bytes(B, H, W)
    if workspace.nbytes < need:
        raise ValueError(f"disp_eval: a workspace of {need} bytes is required, got {workspace.nbytes}")
    d.disp, d.gt, d.workspace, d.stats = disp.data_ptr(), gt.data_ptr(), workspace.data_ptr(), stats.data_ptr()
    d.B, d.H, d.W, d.Hp, d.Wp, d.nthr = B, H, W, Hp, Wp, len(thresholds)
    for i, t in enumerate(thresholds):
        d.thr[i] = t
    d.d1_abs, d.d1_rel, d.gt_min, d.conf_min, d.occ_min = d1_abs, d1_rel, gt_min, conf_min, occ_min
    with torch.cuda.device(disp.device):
        _h._check(_h.load().s2m2_disp_eval(ctypes.byref(d), _h._stream()), "s2m2_disp_eval")
