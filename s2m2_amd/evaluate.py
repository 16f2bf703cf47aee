"""Scoring disparity maps against ground truth on the device (K18, ``s2m2_disp_eval``): EPE, bad-t, D1, RMSE, the A-quantiles, the same after the
confidence / occlusion filter of K15, and the error as a function of the confidence threshold.

``evaluate`` takes the padded maps as ``S2M2.forward`` returns them and the unpadded ground truth, and leaves one block of integer words per pair
on the device (include/s2m2_hip.h: the stat block of K18): two kernel launches, no synchronisation, capturable in a hipGraph.  ``EvalStats``
derives the metrics from the words with plain tensor arithmetic where the words live -- nothing leaves the GPU until ``summary``.  Blocks add:
``a + b`` is the block of both sets of pixels (dataset totals), ``all_reduce`` sums over the ranks of ``shard.py``.

Fixed point: the sum of absolute errors is kept in units of 2^-16 px (every term rounded once, to within 2^-17 px), the sum of squares in units
of 2^-12 px^2, errors from 1024 px on count as 1024 px.  Ratios of empty sets (no evaluated pixel, no finite prediction) are NaN: 0 / 0.

The reference publishes numbers from benchmark servers and has no evaluation code; the semantics here are the header's.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import hip

Q_ABS = 65536.0          # q = rint(min(|e|, 1024) * 2^16)
Q_SQ = 4096.0            # s = rint(min(e^2, 2^20) * 2^12)
HIST_PER_PX = 64.0       # histogram bins per pixel of error


class EvalStats:
    """``words`` (B, hip.EVAL_WORDS) int64, on any device, and the thresholds they were counted with.  Every derived quantity is a (B,) tensor
    (``by_confidence``: (B, 64)) on the device of ``words``; ``kept=True`` selects the pixels that pass conf > conf_min and occ > occ_min."""

    def __init__(self, words: torch.Tensor, thresholds: Sequence[float]):
        if words.dim() != 2 or words.shape[1] != hip.EVAL_WORDS or words.dtype != torch.int64:
            raise ValueError(f"EvalStats: words must be a (B, {hip.EVAL_WORDS}) int64 tensor")
        self.words = words
        self.thresholds = tuple(float(t) for t in thresholds)

    def _block(self, kept: bool) -> torch.Tensor:
        o = hip.EVAL_KEPT if kept else hip.EVAL_ALL
        return self.words[:, o:o + hip.EVAL_BLOCK_WORDS]

    def _slot(self, t: float) -> int:
        if float(t) not in self.thresholds:
            raise KeyError(f"threshold {t} was not counted (thresholds: {self.thresholds})")
        return self.thresholds.index(float(t))

    def count(self, kept: bool = False) -> torch.Tensor:
        """evaluated pixels"""
        return self._block(kept)[:, hip.EVAL_N_EVAL]

    def region(self, kept: bool = False) -> torch.Tensor:
        """pixels of the region, whether their ground truth is valid or not"""
        return self._block(kept)[:, hip.EVAL_N_REGION]

    def nonfinite(self, kept: bool = False) -> torch.Tensor:
        """evaluated pixels whose prediction is inf or NaN"""
        return self._block(kept)[:, hip.EVAL_N_NONFINITE]

    def _finite(self, kept: bool) -> torch.Tensor:
        b = self._block(kept)
        return (b[:, hip.EVAL_N_EVAL] - b[:, hip.EVAL_N_NONFINITE]).double()

    def density(self) -> torch.Tensor:
        """kept / evaluated"""
        return self.count(True).double() / self.count(False).double()

    def epe(self, kept: bool = False) -> torch.Tensor:
        """mean |e| in px over the evaluated pixels with a finite prediction"""
        return self._block(kept)[:, hip.EVAL_SUM_ABS_Q].double() / Q_ABS / self._finite(kept)

    def rmse(self, kept: bool = False) -> torch.Tensor:
        return torch.sqrt(self._block(kept)[:, hip.EVAL_SUM_SQ_Q].double() / Q_SQ / self._finite(kept))

    def bad(self, t: float, kept: bool = False) -> torch.Tensor:
        """share of the evaluated pixels with |e| > t (a prediction that is not finite is bad)"""
        return self._block(kept)[:, hip.EVAL_BAD + self._slot(t)].double() / self.count(kept).double()

    def d1(self, kept: bool = False) -> torch.Tensor:
        return self._block(kept)[:, hip.EVAL_D1_BAD].double() / self.count(kept).double()

    def quantile(self, p: float) -> torch.Tensor:
        """A<100p>: the upper edge, in px, of the 1/64-px histogram bin in which the cumulative count of the evaluated finite pixels first reaches
        p * n; inf when that is the overflow bin (errors of 16 px and more); NaN without pixels"""
        if not 0.0 < p <= 1.0:
            raise ValueError("quantile: 0 < p <= 1")
        hist = self.words[:, hip.EVAL_HIST:hip.EVAL_HIST + hip.EVAL_HIST_BINS]
        cum = hist.cumsum(1).double()
        n = cum[:, -1:]
        first = (cum >= p * n).to(torch.int64).argmax(1)
        edge = (first + 1).double() / HIST_PER_PX
        edge = torch.where(first == hip.EVAL_HIST_BINS - 1, torch.full_like(edge, float("inf")), edge)
        return torch.where(n[:, 0] > 0, edge, torch.full_like(edge, float("nan")))

    def by_confidence(self) -> Dict[str, object]:
        """The filter's trade: column k of every (B, 64) tensor is over the evaluated pixels with conf >= k / 64 (suffix sums of the confidence
        table).  ``density``: their share of the evaluated pixels; ``epe``: sum of |e| / count; ``bad``: {t: share with |e| > t}.  A pair with
        predictions that are not finite has them in the counts and not in the sum of |e| -- read ``nonfinite()`` before ``epe`` here."""
        table = self.words[:, hip.EVAL_CONF:hip.EVAL_CONF + hip.EVAL_CONF_BINS * hip.EVAL_CONF_ROW_WORDS]
        table = table.reshape(-1, hip.EVAL_CONF_BINS, hip.EVAL_CONF_ROW_WORDS)
        suffix = table.flip(1).cumsum(1).flip(1).double()
        count = suffix[:, :, hip.EVAL_CONF_COUNT]
        return {"density": count / self.count(False).double()[:, None],
                "epe": suffix[:, :, hip.EVAL_CONF_SUM_ABS_Q] / Q_ABS / count,
                "bad": {t: suffix[:, :, hip.EVAL_CONF_BAD + i] / count for i, t in enumerate(self.thresholds)}}

    def total(self) -> "EvalStats":
        """the block of all pairs together, (1, WORDS)"""
        return EvalStats(self.words.sum(0, keepdim=True), self.thresholds)

    def __add__(self, other: "EvalStats") -> "EvalStats":
        if not isinstance(other, EvalStats):
            return NotImplemented
        if other.thresholds != self.thresholds:
            raise ValueError("EvalStats: blocks counted with different thresholds do not add")
        return EvalStats(self.words + other.words, self.thresholds)

    def all_reduce(self, dist, group=None) -> "EvalStats":
        """sums the words over the ranks of ``group`` in place: one collective (``dist``: torch.distributed); call it on ``total()`` to move
        WORDS int64 only"""
        dist.all_reduce(self.words, op=dist.ReduceOp.SUM, group=group)
        return self

    def summary(self, b: int = 0) -> dict:
        """plain Python numbers of pair b -- the only method that reads the device (one copy of the pair's words)"""
        host = EvalStats(self.words[b:b + 1].cpu(), self.thresholds)

        def block(kept: bool) -> dict:
            out = {"n_region": int(host.region(kept)[0]), "n_eval": int(host.count(kept)[0]), "nonfinite": int(host.nonfinite(kept)[0]),
                   "epe": float(host.epe(kept)[0]), "rmse": float(host.rmse(kept)[0]), "d1": float(host.d1(kept)[0])}
            out.update({f"bad_{t:g}": float(host.bad(t, kept)[0]) for t in host.thresholds})
            return out

        out = block(False)
        out.update({f"a{round(100 * p)}": float(host.quantile(p)[0]) for p in (0.5, 0.9, 0.95, 0.99)})
        out["density"] = float(host.density()[0])
        out["kept"] = block(True)
        return out


def evaluate(disp: torch.Tensor, gt: torch.Tensor, *, region: Optional[torch.Tensor] = None, occ: Optional[torch.Tensor] = None,
             conf: Optional[torch.Tensor] = None, thresholds: Sequence[float] = (0.5, 1.0, 2.0, 4.0), d1=(3.0, 0.05), gt_min: float = 0.0,
             conf_min: float = 0.1, occ_min: float = 0.5, workspace: Optional[torch.Tensor] = None) -> EvalStats:
    """``disp`` (B,1,Hp,Wp) fp32, padded or not, with ``occ`` and ``conf`` of the same shape or without both; ``gt`` (B,1,H,W) fp32 and ``region``
    (B,1,H,W) uint8 (a pixel takes part where it is not 0), unpadded: the crop of ``image_crop`` is fused.  Ground truth is valid where it is finite
    and > ``gt_min`` (Middlebury / ETH3D mark invalid pixels with inf, KITTI with 0; ``-inf`` accepts every finite value).  Contiguous device
    tensors in, ``EvalStats`` on the device out, no synchronisation.  ``workspace``: ``hip.eval_workspace_bytes(B, H, W)`` bytes to reuse
    between calls (allocated when None)."""
    thresholds = tuple(float(t) for t in thresholds)
    B = disp.shape[0]
    H, W = gt.shape[-2:]
    hip._resident("evaluate", disp, gt, region, occ, conf, workspace)
    if workspace is None:
        workspace = torch.empty((hip.eval_workspace_bytes(B, H, W),), device=disp.device, dtype=torch.uint8)
    words = torch.empty((B, hip.EVAL_WORDS), device=disp.device, dtype=torch.int64)
    hip.disp_eval(disp, gt, words, workspace, region=region, occ=occ, conf=conf, thresholds=thresholds, d1_abs=float(d1[0]), d1_rel=float(d1[1]),
                  gt_min=gt_min, conf_min=conf_min, occ_min=occ_min)
    return EvalStats(words, thresholds)


def read_pfm(path: str) -> np.ndarray:
    """A greyscale PFM file (header ``Pf``, ``width height``, ``scale``; the sign of scale gives the byte order, negative = little-endian; rows
    stored bottom to top) -> (H, W) float32 array, rows top to bottom, values as stored (inf stays inf)."""
    raw = open(path, "rb").read()
    lines, pos = [], 0
    for _ in range(3):
        end = raw.find(b"\n", pos)
        if end < 0:
            raise ValueError(f"{path}: not a PFM file (the header has three lines)")
        lines.append(raw[pos:end].decode("ascii", "replace").strip())
        pos = end + 1
    if lines[0] == "PF":
        raise ValueError(f"{path}: a colour PFM (PF); a disparity map is greyscale (Pf)")
    if lines[0] != "Pf":
        raise ValueError(f"{path}: not a PFM file (magic {lines[0]!r})")
    try:
        width, height = (int(t) for t in lines[1].split())
        scale = float(lines[2])
    except ValueError:
        raise ValueError(f"{path}: malformed PFM header {lines[1]!r} / {lines[2]!r}") from None
    if width <= 0 or height <= 0 or scale == 0.0 or scale != scale:
        raise ValueError(f"{path}: malformed PFM header (width {width}, height {height}, scale {scale})")
    if len(raw) - pos != 4 * width * height:
        raise ValueError(f"{path}: {width} x {height} pixels declared, {len(raw) - pos} bytes of data")
    data = np.frombuffer(raw, dtype="<f4" if scale < 0 else ">f4", offset=pos).reshape(height, width)
    return np.ascontiguousarray(data[::-1]).astype(np.float32)


def write_pfm(path: str, array, little_endian: bool = True) -> None:
    """(H, W) array -> greyscale PFM, scale +-1"""
    a = np.asarray(array, dtype=np.float32)
    if a.ndim != 2 or a.size == 0:
        raise ValueError("write_pfm: a non-empty (H, W) array")
    with open(path, "wb") as f:
        f.write(b"Pf\n%d %d\n%s\n" % (a.shape[1], a.shape[0], b"-1.0" if little_endian else b"1.0"))
        f.write(np.ascontiguousarray(a[::-1]).astype("<f4" if little_endian else ">f4").tobytes())
