"""BASELINE configs[3] (L, CH=256 NTR=3, 1216x1024, refine_iter 3) and configs[4] (XL, CH=384 NTR=3, 2432x2048, allow_negative) against
the REFERENCE itself: tests/golden/e2e_L_1216x1024_fp32_r3_sub.npz / e2e_XL_2432x2048_fp32_r1_neg_sub.npz hold outputs of the
unmodified reference module (tests/golden/make_golden_big.py: sub-sampled transformer features, complete cost-volume rows, complete
DispInit outputs with integer argmax and top-2 relative gap, global-refiner disparity, sub-sampled final maps), in fp32.

GPU (the HIP fp32 forward at these geometries: K1 wide-C strips, K2 with 32 lanes per row at w = 608, K4 at d = 64 / 96 / 256 / 384 and
N = 1216 / 4864 incl. the PE variant with (3, 2) bin tiles, K5 at Cin = 256 ... 768, K9 / K10 or their K5 fallbacks at C = 256 ... 768):

* free running up to DispInit: features / cv at the stage criterion, integer argmax bit exact wherever the reference's own top-2
  relative gap exceeds 1e-4, disp0 / conf0 / occ0 within tolerance except on flipped near ties;
* refinement continued from the reference's own disp0 / conf0 / occ0 (Engine's ``inject`` hook): disp_g and the final maps.

CPU: the file is self-consistent (disp0 follows from argmax + window regression of the stored rows: the oracle's DispInit restatement
reproduces the stored outputs on the stored cost-volume rows) -- a full oracle forward at these sizes takes minutes and is the
reference's job here, not the oracle's."""
import os

import numpy as np
import pytest
import torch

import golden_io
from oracle import s2m2_oracle as O
from s2m2_amd.weights import seeded_state_dict, synthetic_pair

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = {"c4_L": "e2e_L_1216x1024_fp32_r3_sub.npz", "c5_XL": "e2e_XL_2432x2048_fp32_r1_neg_sub.npz"}
ATOL, RTOL = 1e-3, 1e-4


def _load(name):
    g = golden_io.load(FILES[name])
    C, ntr, H, W, B, pos, ri, disparity, seed = [int(v) for v in g["cfg"]]
    return g, dict(C=C, ntr=ntr, H=H, W=W, B=B, pos=bool(pos), ri=ri, disparity=disparity, seed=seed, gain=float(g["gain"]),
                   sub=int(g["sub"]), fsub=int(g["fsub"]), cvsub=int(g["cvsub"]), gsub=int(g["gsub"]))


def _sure(g, c, cv_err=0.0):
    """Pixels whose integer argmax must be reproduced bit for bit: the reference's own top-2 relative gap of the masked transport
    probabilities exceeds what fp32 summation order of the correlation sums can move.  P ~ exp(S + ...): an error e in two scores moves
    the relative gap by up to 2e, so the threshold is max(1e-4, 4 x the largest cost-volume error measured in this test) -- 1e-4 at
    C = 128 (|cv| ~ 128, errors ~1e-4), ~2e-3 at C = 384 (|cv| ~ 380: one fp32 ulp is 3e-5, sums of 384 terms differ by ~5e-4)."""
    return torch.as_tensor(g["gap0"].astype(np.float32))[:, 0] > max(1e-4, 4.0 * cv_err)


def _t(a):
    return torch.as_tensor(np.asarray(a)).float()


def _frac_out(test, ref):
    d = (test.float() - ref.float()).abs()
    return float((d > ATOL + RTOL * ref.float().abs()).float().mean()), float(d.max()), float(d.median())


@pytest.mark.parametrize("name", list(FILES))
def test_golden_rows_are_reproduced_by_the_oracles_dispinit(name):
    """Sinkhorn + argmax + window regression of the oracle (the checker of every K2 operator test, incl. w = 608) on the stored
    reference cost-volume rows vs the stored reference outputs of those rows."""
    g, c = _load(name)
    cv = _t(g["cv"])
    rows = slice(None, None, c["cvsub"])
    P = O.sinkhorn_prob(cv, c["pos"])
    d, cf, oc, ind = O.regress(P)
    sure = _sure(g, c, 1e-4)[:, rows]                       # (the oracle runs on the reference's own cv rows: only the OT sums differ)
    am_ref = torch.as_tensor(g["argmax"].astype(np.int32))[:, rows]
    assert bool((ind.int() == am_ref)[sure].all()) and float(sure.float().mean()) > 0.99
    same = ind.int() == am_ref
    assert float((d[:, 0] - _t(g["disp0"])[:, 0, rows]).abs()[same].max()) < 2e-4 + 2e-7 * cv.shape[-1]
    assert float((cf[:, 0] - _t(g["conf0"])[:, 0, rows]).abs()[same].max()) < 5e-5
    assert float((oc[:, 0] - _t(g["occ0"])[:, 0, rows]).abs().max()) < 5e-5


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FILES))
def test_hip_fp32_against_the_reference(name):
    import parity_util as PU
    g, c = _load(name)
    sd = seeded_state_dict(c["C"], 1, c["ntr"], c["seed"], gain=c["gain"])
    left, right = synthetic_pair(c["H"], c["W"], c["B"], c["disparity"], c["seed"])
    hout, hcap = PU.hip_forward(sd, c["C"], c["ntr"], c["ri"], left, right, False, use_positivity=c["pos"])
    report = {}
    # ---- free running up to DispInit
    f = hcap["feature_tr_4x"][:, :, ::c["fsub"], ::c["fsub"]]
    report["feature_tr_4x"] = _frac_out(f, _t(g["feature_tr_4x"]))
    assert report["feature_tr_4x"][0] <= 1e-3, report
    report["cv"] = _frac_out(hcap["cv"][:, ::c["cvsub"]], _t(g["cv"]))
    assert report["cv"][0] <= 1e-3, report
    am_ref = torch.as_tensor(g["argmax"].astype(np.int32))
    same = hcap["argmax"].int() == am_ref
    sure = _sure(g, c, report["cv"][1])
    report["argmax"] = (float(same.float().mean()), float(sure.float().mean()), int((~same[sure]).sum()))
    assert report["argmax"][2] == 0 and report["argmax"][0] >= 0.995, report
    flipped = 1.0 - report["argmax"][0]
    for k in ("disp0", "conf0", "occ0"):
        report[k] = _frac_out(hcap[k], _t(g[k]))
        assert report[k][0] <= flipped + 1e-4, report
    # ---- refinement from the reference's own DispInit outputs
    inj = {k: _t(g[k]) for k in ("disp0", "conf0", "occ0")}
    hout, hcap2 = PU.hip_forward(sd, c["C"], c["ntr"], c["ri"], left, right, False, inject=inj, use_positivity=c["pos"])
    report["disp_g"] = _frac_out(hcap2["disp_g"][..., ::c["gsub"], ::c["gsub"]], _t(g["disp_g"]))
    assert report["disp_g"][0] <= 1e-3, report
    sub = c["sub"]
    for k, nm in enumerate(("disp", "occ", "conf")):
        report[nm] = _frac_out(hout[k][..., ::sub, ::sub], _t(g[nm]))
        assert torch.isfinite(hout[k]).all()
        assert report[nm][0] <= 2e-3, report
    print(name, report)
