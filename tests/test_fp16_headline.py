"""BASELINE.json's configurations IN THE PRECISION THEY ARE STATED IN (fp16, the mode bench.py times), end to end, at their own sizes:

  c3  S  (C 128, NTR 1) 1216x1024 refine_iter 3 use_positivity        -- the headline workload of bench.py
  c4  L  (C 256, NTR 3) 1216x1024 refine_iter 3 use_positivity
  c5  XL (C 384, NTR 3) 2432x2048 refine_iter 3 allow_negative
  m   M  (C 192, NTR 2)  640x480  refine_iter 3 use_positivity        -- the width without a folded-LayerNorm K1 / direct K9 path

Checker: outputs of the UNMODIFIED reference (tests/golden/make_golden_fp16_big.py -> e2e_*_fp16_r3_sub.npz): its fp32 run and its run
under ``torch.amp.autocast(float16)`` the way run_stereo_matching deploys it (model_utils.py:75-76, device cpu in the build container);
for c3 additionally the oracle's autocast emulation executed inside the test (the op-level policy of CUDA autocast).

Two legs per configuration:

* SHARP (tight): ``feature_tr_4x`` replaced on both sides by synthetic tokens with one unambiguous match per pixel (top-2 gap 1.0), no
  positivity mask.  No argmax can flip, so everything downstream of the injection point is held tight in fp16: integer argmax BIT EXACT,
  cost volume within one fp16 ulp of the reference's fp16 einsum, DispInit within the reference's own fp16 quantisation, final maps no
  further from the reference's fp16 run than that run is from the reference's fp32 run.  The injected tokens go through the shipped
  launch pair (K9 LayerNorm output -> s2m2_corr: Engine._normed_like_the_forward), i.e. the kernel bench.py's roofline line measures, at
  the geometry it measures it at (256 x 304 x 128 for c3).
* NATURAL (statistical): the free-running fp16 forward on the seeded textured pair -- every fp16-only fast path of the engine (direct K9 /
  K10, fragment-stream K5, merged GRU gates, pooled / fan-out launches) composed at 256x304 ... 32x38 -- must sit as close to the
  reference's fp16 maps as the reference's own fp32 run does (near-tie argmax flips make two fp16 runs differ by px on a few percent of
  the pixels: the reference's fp16-vs-fp32 distance is the yardstick: margin 1.5 on median / p90, 2.5 on p99, see _inside_spread), and
  must be no less accurate against the reference's FP32 maps than the reference's own fp16 run is.

fp32 legs added with the same goldens: c5 at refine_iter 3 (continued from the reference's DispInit outputs of the r1 golden: same weights
and pair) and M 640x480 (every stage vs the oracle, finals vs the reference)."""
import os

import numpy as np
import pytest
import torch

import golden_io
from oracle import s2m2_oracle as O
from s2m2_amd.weights import seeded_state_dict, synthetic_pair

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = {"c3": "e2e_S_1216x1024_fp16_r3_sub.npz", "c4": "e2e_L_1216x1024_fp16_r3_sub.npz", "c5": "e2e_XL_2432x2048_fp16_r3_sub.npz",
         "m": "e2e_M_640x480_fp16_r3_sub.npz"}
MARGIN = 1.5


def _load(name):
    g = golden_io.load(FILES[name])
    C, ntr, H, W, B, pos, ri, disparity, seed = [int(v) for v in g["cfg"]]
    return g, dict(C=C, ntr=ntr, H=H, W=W, B=B, pos=bool(pos), ri=ri, disparity=disparity, seed=seed, gain=float(g["gain"]), sub=int(g["sub"]),
                   sub0=int(g["sub0"]), cvsub=int(g["cvsub"]), shifts=tuple(int(v) for v in g["shifts"]), tok_seed=int(g["tok_seed"]))


def _t(a):
    return torch.as_tensor(np.asarray(a)).float()


def _q(d, p):
    d = d.flatten()
    return float(d.kthvalue(max(1, min(d.numel(), int(round(p * d.numel())))))[0])


def _dist(a, b):
    d = (_t(a) - _t(b)).abs()
    return dict(median=float(d.median()), p90=_q(d, 0.9), p99=_q(d, 0.99), max=float(d.max()))


def _inside_spread(mine, ref16, ref32, what, margin=MARGIN, eps=1e-4, tail=None):
    """|mine - ref16| no larger than margin x |ref16 - ref32| at the median and p90, and ``tail`` x at p99.  Two fp16 runs are two independent
    perturbations of the fp32 run: in the bulk their distance is ~sqrt(2) x one perturbation (margin 1.5); the p99 tail is made of the pixels
    behind near-tie argmax flips, and the flips of two runs are disjoint sets -- twice as many pixels as the yardstick's, so the p99 quantile
    reaches deeper into the same tail (tail margin 2.5)."""
    m, y = _dist(mine, ref16), _dist(ref16, ref32)
    for k in ("median", "p90", "p99"):
        mg = (tail if tail is not None else max(margin, 2.5)) if k == "p99" else margin
        assert m[k] <= mg * y[k] + eps, f"{what} {k}: {m[k]:.4g} vs the reference's fp16-fp32 distance {y[k]:.4g} (margin {mg})"
    return m, y


def _ulp16(x, floor=2.0 ** -14):
    """one fp16 ulp at max(|x|, floor)"""
    return torch.pow(2.0, torch.floor(torch.log2(x.abs().clamp_min(floor))) - 10)


def _report(tag, rep):
    """measured statistics of a leg -> gpurun_out/fp16_headline/<tag>.json (kept as profiles/r04/fp16_headline_*.json) and stdout"""
    import json
    print(tag, json.dumps(rep, default=float))
    d = os.path.join(os.path.dirname(HERE), "gpurun_out", "fp16_headline")
    try:
        os.makedirs(d, exist_ok=True)
        json.dump(rep, open(os.path.join(d, tag + ".json"), "w"), indent=1, default=float)
    except OSError:
        pass


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the goldens are self-consistent and pin the oracle's injected / fp16 paths
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FILES))
def test_goldens_are_self_consistent(name):
    g, c = _load(name)
    assert bool((g["s_argmax_16"] == g["s_argmax_32"]).all()) and float(g["s_mingap_32"]) > 0.5 and float(g["s_mingap_16"]) > 0.5
    h, w = c["H"] // 4, c["W"] // 4
    assert g["s_argmax_32"].shape == (1, h, w) and g["s_cv_16"].dtype == np.float16 and g["s_cv_16"].shape[2:] == (w, w)
    # the sharp construction: left pixel i matches right pixel (i - shift) mod w in its row band
    band = (h + len(c["shifts"]) - 1) // len(c["shifts"])
    for k, d in enumerate(c["shifts"]):
        rows = slice(k * band, min(h, (k + 1) * band))
        want = (np.arange(w) - d) % w
        assert bool((g["s_argmax_32"][0, rows] == want[None]).all())
    for k in ("n_disp_16", "n_disp_32", "s_disp_16", "s_disp_32"):
        assert np.isfinite(g[k]).all() and g[k].shape == (1, 1, c["H"] // c["sub"], c["W"] // c["sub"])


def test_oracle_finish_stages_from_injected_tokens_match_the_reference_M():
    """oracle (fp32) with the sharp tokens injected vs the reference's own run with the same tokens: pins DispInit + refiners + upsampling
    of the oracle at C = 192 behind the injection hook; and its fp16 emulation inside the reference's own fp16-vs-fp32 spread."""
    import parity_util as PU
    g, c = _load("m")
    torch.set_num_threads(min(8, torch.get_num_threads()))
    sd = seeded_state_dict(c["C"], 1, c["ntr"], c["seed"], gain=c["gain"])
    left, right = synthetic_pair(c["H"], c["W"], 1, c["disparity"], c["seed"])
    tok = PU.sharp_tokens(c["C"], c["H"] // 4, c["W"] // 4, c["shifts"], c["tok_seed"])
    cap = {}
    out = O.forward(sd, left, right, False, c["ri"], False, cap, inject={"feature_tr_4x": tok})
    assert bool((cap["argmax"].int() == torch.as_tensor(g["s_argmax_32"].astype(np.int32))).all())
    assert float((cap["disp0"] - _t(g["s_disp0_32"])).abs().max()) < 1e-3
    sub = c["sub"]
    for k, nm in enumerate(("disp", "occ", "conf")):
        ref = _t(g[f"s_{nm}_32"])
        e = (out[k][..., ::sub, ::sub] - ref).abs()
        assert float((e > 1e-3 + 1e-4 * ref.abs()).float().mean()) <= 1e-3, (nm, float(e.max()))      # (occ / conf stored as fp16: 5e-4 resolution)
    o16 = O.forward(sd, left, right, False, c["ri"], False, {}, precision="fp16", inject={"feature_tr_4x": tok})
    for k, nm in enumerate(("disp", "occ", "conf")):
        _inside_spread(o16[k][..., ::sub, ::sub], g[f"s_{nm}_16"], g[f"s_{nm}_32"], f"oracle fp16 sharp {nm}", eps=1e-3)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _hip(c, left, right, fp16, inject=None, pos=None):
    import parity_util as PU
    sd = seeded_state_dict(c["C"], 1, c["ntr"], c["seed"], gain=c["gain"])
    return PU.hip_forward(sd, c["C"], c["ntr"], c["ri"], left, right, fp16, inject=inject, use_positivity=c["pos"] if pos is None else pos)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FILES))
def test_natural_fp16_forward_inside_the_references_own_fp16_spread(name):
    g, c = _load(name)
    left, right = synthetic_pair(c["H"], c["W"], 1, c["disparity"], c["seed"])
    hout, _ = _hip(c, left, right, True)
    assert all(torch.isfinite(t).all() for t in hout)
    sub = c["sub"]
    rep = {}
    for k, nm in enumerate(("disp", "occ", "conf")):
        mine = hout[k][..., ::sub, ::sub]
        rep[nm] = dict(hip16_vs_ref16=_dist(mine, g[f"n_{nm}_16"]), ref16_vs_ref32=_dist(g[f"n_{nm}_16"], g[f"n_{nm}_32"]),
                       hip16_vs_ref32=_dist(mine, g[f"n_{nm}_32"]))
    _report(f"natural_{name}", rep)
    for k, nm in enumerate(("disp", "occ", "conf")):
        _inside_spread(hout[k][..., ::sub, ::sub], g[f"n_{nm}_16"], g[f"n_{nm}_32"], f"{name} HIP fp16 natural {nm}")
        # and measured against the reference's FP32 maps the HIP fp16 forward is no less accurate than the reference's own fp16 deployment
        a, y = rep[nm]["hip16_vs_ref32"], rep[nm]["ref16_vs_ref32"]
        assert a["median"] <= 1.25 * y["median"] + 1e-4 and a["p90"] <= 1.5 * y["p90"] + 1e-4, (name, nm, a, y)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FILES))
def test_sharp_fp16_forward_tight_against_the_references_fp16_run(name):
    import parity_util as PU
    g, c = _load(name)
    h, w = c["H"] // 4, c["W"] // 4
    left, right = synthetic_pair(c["H"], c["W"], 1, c["disparity"], c["seed"])
    tok = PU.sharp_tokens(c["C"], h, w, c["shifts"], c["tok_seed"])
    hout, hcap = _hip(c, left, right, True, inject={"feature_tr_4x": tok}, pos=False)
    assert all(torch.isfinite(t).all() for t in hout)
    # integer argmax: bit exact (the reference's fp16 and fp32 runs agree with each other too)
    assert bool((hcap["argmax"].int() == torch.as_tensor(g["s_argmax_16"].astype(np.int32))).all()), "integer argmax must be bit exact when no near tie exists"
    # cost volume: the reference's autocast einsum (fp16 operands, one rounding of the fp32 sum) on its fp32 LayerNorm rounded to fp16
    ref_cv = _t(g["s_cv_16"])
    d = (hcap["cv"][:, ::c["cvsub"]].float() - ref_cv).abs()
    # one fp16 ulp of the value; near zero (|cv| < 16: ulp < 2^-6) the two fp32 sums of C products of magnitude ~1 differ by their
    # summation order before the rounding, so the floor of the bound is the ulp at 16
    ulp = _ulp16(ref_cv, floor=16.0)
    assert bool((d <= ulp).all()), (float(d.max()), float((d / ulp).max()))
    assert float((d > 0).float().mean()) <= 2e-2, float((d > 0).float().mean())     # (measured 0.4 % at C = 128 ... 0.75 % at C = 192: single-ulp differences)
    # DispInit: K2 keeps fp32 where autocast rounds the probabilities and the 5-tap window to fp16 -> within the fp16 quantisation of |j| <= w
    s0 = (slice(None), slice(None), slice(None, None, c["sub0"]), slice(None, None, c["sub0"]))
    qd = float(_ulp16(torch.tensor(float(w - 1))))
    e16 = (hcap["disp0"][s0] - _t(g["s_disp0_16"])).abs()
    e32 = (hcap["disp0"][s0] - _t(g["s_disp0_32"])).abs()
    y = (_t(g["s_disp0_16"]) - _t(g["s_disp0_32"])).abs()
    assert float(e16.max()) <= 1.3 * qd and float(e32.max()) <= max(float(y.max()), 0.05), (float(e16.max()), float(e32.max()), float(y.max()), qd)
    assert float((hcap["conf0"][s0] - _t(g["s_conf0_16"])).abs().max()) <= 4e-3 and float((hcap["occ0"][s0] - _t(g["s_occ0_16"])).abs().max()) <= 4e-3
    # final maps, free running from the injection point: no discrete decision is left
    sub = c["sub"]
    rep = {}
    for k, nm in enumerate(("disp", "occ", "conf")):
        rep[nm] = _inside_spread(hout[k][..., ::sub, ::sub], g[f"s_{nm}_16"], g[f"s_{nm}_32"], f"{name} HIP fp16 sharp {nm}", eps=1e-3, tail=1.5)
        rep[nm + "_vs_fp32"] = _dist(hout[k][..., ::sub, ::sub], g[f"s_{nm}_32"])
    rep["cv"] = dict(max=float(d.max()), frac_differing=float((d > 0).float().mean()))
    rep["disp0"] = dict(vs_ref16=float(e16.max()), vs_ref32=float(e32.max()), ref16_vs_ref32=float(y.max()), fp16_quantum=qd)
    _report(f"sharp_{name}", {k: (v if isinstance(v, dict) else dict(hip16_vs_ref16=v[0], ref16_vs_ref32=v[1])) for k, v in rep.items()})
    # the HIP fp16 forward keeps fp32 where autocast rounds between ops: it must be closer to the reference's FP32 run than the reference's fp16 run is
    yd = _dist(g["s_disp_16"], g["s_disp_32"])
    assert rep["disp_vs_fp32"]["median"] <= yd["median"] + 1e-3 and rep["disp_vs_fp32"]["p99"] <= yd["p99"] + 1e-2, (rep["disp_vs_fp32"], yd)


@pytest.mark.gpu
def test_c3_fp16_headline_against_the_autocast_emulation():
    """The headline workload (S 1216x1024 fp16 refine_iter 3) against the oracle's emulation of CUDA autocast, executed here:
    (a) sharp tokens at 256 x 304: integer argmax bit exact, cv <= 1 fp16 ulp, free-running finals within 1.15 x the emulation-vs-fp32 spread;
    (b) teacher forced on the natural pair: K1 + K2 from the emulation's features, and every stage after DispInit from the emulation's
        cv / disp0 / conf0 / occ0."""
    import parity_util as PU
    g, c = _load("c3")
    ri, h, w = c["ri"], c["H"] // 4, c["W"] // 4
    torch.set_num_threads(min(32, torch.get_num_threads()))
    sd = seeded_state_dict(c["C"], 1, c["ntr"], c["seed"], gain=c["gain"])
    left, right = synthetic_pair(c["H"], c["W"], 1, c["disparity"], c["seed"])
    # ---- (a)
    tok = PU.sharp_tokens(c["C"], h, w, c["shifts"], c["tok_seed"])
    c16, c32 = {}, {}
    o16 = O.forward(sd, left, right, False, ri, False, c16, precision="fp16", inject={"feature_tr_4x": tok})
    o32 = O.forward(sd, left, right, False, ri, False, c32, precision="fp32", inject={"feature_tr_4x": tok})
    assert bool((c16["argmax"] == c32["argmax"]).all()) and bool((c32["argmax"].int() == torch.as_tensor(g["s_argmax_32"].astype(np.int32))).all())
    hout, hcap = _hip(c, left, right, True, inject={"feature_tr_4x": tok}, pos=False)
    assert bool((hcap["argmax"].long() == c16["argmax"].long()).all())
    rows, _ = PU.compare(hcap, hout, c16, o16, ri)
    ref_rows, _ = PU.compare(c16, o16, c32, o32, ri)
    names = ["disp", "occ", "conf", f"disp_it{ri - 1}"]
    st, ref = PU.select(rows, ["cv", "disp0", "conf0", "occ0"] + names), PU.select(ref_rows, names)
    assert st["cv"]["max"] <= 0.125 and st["disp0"]["max"] <= 1.3 * 0.25 and st["conf0"]["max"] <= 4e-3 and st["occ0"]["max"] <= 4e-3, st
    for nm in names:
        assert st[nm]["median"] <= 1.15 * ref[nm]["median"] + 1e-4 and st[nm]["p99"] <= 1.15 * ref[nm]["p99"] + 1e-3, (nm, st[nm], ref[nm])
    _report("c3_sharp_vs_emulation", dict(hip16_vs_emulation={k: dict(median=v["median"], p99=v["p99"], max=v["max"]) for k, v in st.items()},
                                          emulation_vs_fp32={k: dict(median=v["median"], p99=v["p99"], max=v["max"]) for k, v in ref.items()}))
    # ---- (b)
    n16 = {}
    on16 = O.forward(sd, left, right, True, ri, False, n16, precision="fp16")
    h2, hc2 = _hip(c, left, right, True, inject={"feature_tr_4x": n16["feature_tr_4x"]})
    r2, am2 = PU.compare(hc2, h2, n16, on16, ri)
    d = (hc2["cv"].float() - n16["cv"].float()).abs()
    assert float(d.max()) <= 0.125 and float((d > 0).float().mean()) <= 2e-3, (float(d.max()), float((d > 0).float().mean()))
    assert am2["agree_all"] >= 0.998, am2
    inj = {k: n16[k] for k in ("cv", "disp0", "conf0", "occ0")}
    h3, hc3 = _hip(c, left, right, True, inject=inj)
    r3, _ = PU.compare(hc3, h3, n16, on16, ri)
    s3 = PU.select(r3, ["disp", "occ", "conf", f"disp_it{ri - 1}"])
    # yardstick: the reference's own fp16 run against its fp32 run on this pair (golden).  At this geometry the disparities reach 1160 px
    # (290 at 1/4 resolution, where autocast holds them in fp16: quantum 0.25) and the randomly initialised refiners amplify rounding noise:
    # the reference's two runs differ by 0.78 px at the median.  The HIP forward continued from the emulation's DispInit outputs has no
    # argmax flips to account for, so the full-resolution maps must sit INSIDE that spread (no margin)
    sub = c["sub"]
    yard = {nm: _dist(g[f"n_{nm}_16"], g[f"n_{nm}_32"]) for nm in ("disp", "occ", "conf")}
    _report("c3_teacher_forced", dict(hip16_vs_emulation={k: dict(median=v["median"], p99=v["p99"], max=v["max"]) for k, v in s3.items()},
                                      ref16_vs_ref32=yard, k1_k2=dict(cv_max=float(d.max()), cv_frac_differing=float((d > 0).float().mean()), **am2)))
    for nm in ("disp", "occ", "conf"):
        assert s3[nm]["median"] <= yard[nm]["median"] + 1e-4 and s3[nm]["p99"] <= yard[nm]["p99"] + 1e-3, (nm, s3[nm], yard[nm])
    # (the last iteration's 1/4-resolution disparity -- ONE realisation of amplified rounding noise per pair, 0.1947 / 0.1957 / 0.1908 / 0.1920 in
    # rounds 4 - 6 against a yardstick / 4 of 0.1946 -- is judged on an ensemble of three pairs: test_c3_fp16_teacher_forced_ensemble)


@pytest.mark.gpu
def test_c3_fp16_teacher_forced_ensemble():
    """The teacher-forced statistics of the headline workload as a MEAN over three seeded pairs, so that a change of summation order upstream
    cannot flip the test either way.  Per pair: the oracle's autocast emulation (fp16) and the oracle in fp32, both free running on the natural
    pair -> the yardstick (how far the fp16 deployment sits from fp32 on this pair, after three refinement iterations with randomly initialised
    refiners); the HIP fp16 forward continued from the emulation's cv / disp0 / conf0 / occ0 against the emulation.  Bound: no margin on the
    means, at full resolution (disp) and at 1/4 resolution before the upsampling head (disp_it{last})."""
    import parity_util as PU
    g, c = _load("c3")
    ri = c["ri"]
    torch.set_num_threads(min(32, torch.get_num_threads()))
    sd = seeded_state_dict(c["C"], 1, c["ntr"], c["seed"], gain=c["gain"])
    names = ["disp", f"disp_it{ri - 1}"]
    mine = {n: [] for n in names}
    yard = {n: [] for n in names}
    per_pair = []
    for k in range(3):
        left, right = synthetic_pair(c["H"], c["W"], 1, c["disparity"], c["seed"] + k)
        n16, n32 = {}, {}
        on16 = O.forward(sd, left, right, True, ri, False, n16, precision="fp16")
        on32 = O.forward(sd, left, right, True, ri, False, n32, precision="fp32")
        h3, hc3 = _hip(c, left, right, True, inject={key: n16[key] for key in ("cv", "disp0", "conf0", "occ0")})
        r3, _ = PU.compare(hc3, h3, n16, on16, ri)
        ry, _ = PU.compare(n16, on16, n32, on32, ri)
        s3, sy = PU.select(r3, names), PU.select(ry, names)
        for n in names:
            mine[n].append(s3[n]["median"])
            yard[n].append(sy[n]["median"])
        per_pair.append(dict(seed=c["seed"] + k, hip16_vs_emulation={n: s3[n]["median"] for n in names}, emulation_vs_fp32={n: sy[n]["median"] for n in names}))
    mean = lambda v: sum(v) / len(v)                                  # noqa: E731
    _report("c3_teacher_forced_ensemble", dict(pairs=per_pair, mean_hip16_vs_emulation={n: mean(mine[n]) for n in names},
                                               mean_emulation_vs_fp32={n: mean(yard[n]) for n in names},
                                               golden_ref16_vs_ref32_pair0=_dist(g["n_disp_16"], g["n_disp_32"])["median"]))
    for n in names:
        assert mean(mine[n]) <= mean(yard[n]) + 1e-4, (n, mine[n], yard[n])


@pytest.mark.gpu
def test_web0025_full_size_fp16_against_the_references_cpu_autocast_run():
    """The reference's own sample pair data/samples/Web/0025_{L,R}.png at its natural size (1100 x 800, padded to 1120 x 800 by image_pad), S model,
    refine_iter 3, fp16: image_pad -> forward under autocast -> image_crop (the body of run_stereo_matching, model_utils.py:69-94) against the
    golden of the reference's CPU-autocast run of the same body, with the reference's fp32 run as the yardstick (tests/golden/make_golden_web_fp16.py)."""
    from s2m2_amd import utils
    from s2m2_amd.model import S2M2
    g = golden_io.load("e2e_S_web0025_full_fp16_r3.npz")
    C, ntr, H, W, _, pos, ri, _, seed = [int(v) for v in g["cfg"]]
    left = torch.from_numpy(g["left"]).permute(2, 0, 1)[None].cuda()
    right = torch.from_numpy(g["right"]).permute(2, 0, 1)[None].cuda()
    m = S2M2(C, 1, ntr, use_positivity=bool(pos), refine_iter=ri)
    m.load_state_dict(seeded_state_dict(C, 1, ntr, seed), strict=True)
    m = m.cuda().eval()
    lp, rp = utils.image_pad(left, 32), utils.image_pad(right, 32)
    assert tuple(lp.shape[-2:]) == tuple(int(v) for v in g["padded"])
    with torch.inference_mode(), torch.autocast("cuda", dtype=torch.float16):
        out = m(lp, rp)
    d, o, c = (utils.image_crop(t, (H, W)).squeeze().float().cpu() for t in out)
    assert tuple(d.shape) == (H, W) and all(torch.isfinite(t).all() for t in (d, o, c))
    rep = {}
    for nm, t in (("disp", d), ("occ", o), ("conf", c)):
        rep[nm] = dict(hip16_vs_ref16=_dist(t[::2, ::2], g[f"{nm}_fp16"]), ref16_vs_ref32=_dist(g[f"{nm}_fp16"], g[f"{nm}_fp32"]),
                       hip16_vs_ref32=_dist(t[::2, ::2], g[f"{nm}_fp32"]))
    score = float(c[100:-100, 100:-100].mean())
    rep["avg_conf"] = dict(hip16=score, ref16=float(g["avg_conf_fp16"]), ref32=float(g["avg_conf_fp32"]))
    _report("web0025_full_fp16", rep)
    for nm, t in (("disp", d), ("occ", o), ("conf", c)):
        _inside_spread(t[::2, ::2], g[f"{nm}_fp16"], g[f"{nm}_fp32"], f"web0025 HIP fp16 {nm}", eps=2e-3)
    assert abs(score - float(g["avg_conf_fp16"])) <= max(3 * abs(float(g["avg_conf_fp16"]) - float(g["avg_conf_fp32"])), 2e-3), rep["avg_conf"]


@pytest.mark.gpu
def test_c5_fp32_refine_iter_3_against_the_reference():
    """BASELINE configs[4] at its own refine_iter (the r1 golden of make_golden_big.py covers DispInit; same weights and pair): the HIP fp32
    forward continued from the reference's disp0 / conf0 / occ0 vs the reference's fp32 maps after three refinement iterations."""
    g, c = _load("c5")
    g1 = golden_io.load("e2e_XL_2432x2048_fp32_r1_neg_sub.npz")
    assert [int(v) for v in g1["cfg"]][:6] == [c["C"], c["ntr"], c["H"], c["W"], 1, 0] and [int(v) for v in g1["cfg"]][7:] == [c["disparity"], c["seed"]]
    assert float(g1["gain"]) == c["gain"]
    left, right = synthetic_pair(c["H"], c["W"], 1, c["disparity"], c["seed"])
    hout, _ = _hip(c, left, right, False, inject={k: _t(g1[k]) for k in ("disp0", "conf0", "occ0")})
    sub = c["sub"]
    rep = {}
    for k, nm in enumerate(("disp", "occ", "conf")):
        ref = _t(g[f"n_{nm}_32"])
        e = (hout[k][..., ::sub, ::sub] - ref).abs()
        atol = 1e-3 if nm == "disp" else 1.5e-3                      # occ / conf are stored as fp16 (resolution 4.9e-4 below 1)
        rep[nm] = (float((e > atol + 1e-4 * ref.abs()).float().mean()), float(e.max()), int((e > 1e-3).sum()))
        assert rep[nm][0] <= 2e-3, rep
    _report("c5_fp32_r3_vs_reference", {k: dict(frac_out=v[0], max=v[1], n_abs_gt_1e3=v[2]) for k, v in rep.items()})
    assert rep["disp"][1] < 0.1, rep


@pytest.mark.gpu
def test_m_640x480_fp32_every_stage_and_against_the_reference():
    """M (C 192, NTR 2; head dims 96 / 48 / 24; no folded-LayerNorm K1, K9 / K10 fall back to K5 launches) at a real size: every stage vs the
    oracle executed here, finals vs the reference's own fp32 maps."""
    import parity_util as PU
    g, c = _load("m")
    ri = c["ri"]
    torch.set_num_threads(min(32, torch.get_num_threads()))
    sd = seeded_state_dict(c["C"], 1, c["ntr"], c["seed"], gain=c["gain"])
    left, right = synthetic_pair(c["H"], c["W"], 1, c["disparity"], c["seed"])
    ocap = {}
    oout = O.forward(sd, left, right, True, ri, False, ocap)
    hout, hcap = _hip(c, left, right, False)
    rows, am = PU.compare(hcap, hout, ocap, oout, ri)
    assert am["mismatch_sure"] == 0 and am["agree_all"] >= 0.999, am
    if am["agree_all"] < 1.0:
        hout, hcap2 = _hip(c, left, right, False, inject={k: ocap[k] for k in ("disp0", "conf0", "occ0")})
        rows2, _ = PU.compare(hcap2, hout, ocap, oout, ri)
        keep = {"feature_py_4x", "feature_tr_4x", "cv", "ctx"}
        rows = [r for r in rows if r[0] in keep] + [r for r in rows2 if r[0] not in keep and not r[0].endswith("0")]
    for name, _, s in rows:
        lim = 1e-2 if name.startswith("corr") else 1e-3
        assert s["finite"] and s["frac_out"] <= lim, (name, s)
    sub = c["sub"]
    for k, nm in enumerate(("disp", "occ", "conf")):
        ref = _t(g[f"n_{nm}_32"])
        e = (hout[k][..., ::sub, ::sub] - ref).abs()
        atol = 1e-3 if nm == "disp" else 1.5e-3
        assert float((e > atol + 1e-4 * ref.abs()).float().mean()) <= 2e-3, (nm, float(e.max()))
