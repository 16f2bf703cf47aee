"""numpy oracle of K18 (include/s2m2_hip.h: s2m2_disp_eval): the per-pixel rules of the header restated with np.float32 arithmetic and Python
integers, and a float64 "textbook" EPE / RMSE / bad-t over the same pixels.  Nothing here imports the code under test; the layout constants are
restated too (tests/test_eval_cpu.py compares them with the header's and the binding's)."""
import numpy as np

MAX_THR, HIST_BINS, CONF_BINS = 8, 1025, 64
N_REGION, N_EVAL, N_NONFINITE, SUM_ABS_Q, SUM_SQ_Q, D1_BAD, BAD, BLOCK_WORDS = 0, 1, 2, 3, 4, 5, 6, 14
CONF_COUNT, CONF_SUM_ABS_Q, CONF_BAD, CONF_ROW_WORDS = 0, 1, 2, 10
ALL, KEPT, HIST, CONF = 0, 14, 28, 1053
WORDS = CONF + CONF_BINS * CONF_ROW_WORDS            # 1693

F = np.float32


def crop(m, H, W):
    """the window image_crop cuts out of a padded (..., Hp, Wp) map"""
    Hp, Wp = m.shape[-2:]
    oy, ox = (Hp - H) // 2, (Wp - W) // 2
    return m[..., oy:oy + H, ox:ox + W]


def draw(B, Hp, Wp, H, W, seed, ties=(0.5, 1.0, 2.0, 3.0, 4.0)):
    """Test inputs: padded maps (B,1,Hp,Wp) -- disparity uniform in [-20, 300], conf / occ uniform in [0, 1] -- and, for the (H, W) window
    image_crop cuts out, gt = prediction + noise of mixed scale (0.01 .. 30 px, both signs) with about 10 % inf and 5 % <= 0, and a region with
    about 20 % zeros.  Knife edges on purpose: about 3 % of the pixels have an integer gt and a prediction exactly `ties` px above it.
    -> dict of float32 / uint8 arrays"""
    g = np.random.default_rng(seed)
    disp = (g.random((B, 1, Hp, Wp), dtype=F) * F(320) - F(20)).astype(F)
    conf, occ = g.random((B, 1, Hp, Wp), dtype=F), g.random((B, 1, Hp, Wp), dtype=F)
    win = crop(disp, H, W)                                           # a view: the ties below are written into disp
    noise = (F(10) ** (g.random((B, 1, H, W), dtype=F) * F(3.48) - F(2))) * g.choice(np.array([-1, 1], dtype=F), (B, 1, H, W))
    gt = (win + noise).astype(F)
    tie = g.random((B, 1, H, W)) < 0.03
    k = np.rint(np.abs(gt[tie])) + F(1)
    gt[tie] = k
    win[tie] = k + g.choice(np.array(ties, dtype=F), k.shape)
    u = g.random((B, 1, H, W))
    gt[u < 0.10] = np.inf
    gt[(u >= 0.10) & (u < 0.13)] = 0.0
    gt[(u >= 0.13) & (u < 0.15)] *= F(-1)
    region = (g.random((B, 1, H, W)) >= 0.2).astype(np.uint8) * g.integers(1, 256, (B, 1, H, W), dtype=np.uint8)
    return dict(disp=disp, occ=occ, conf=conf, gt=gt, region=region)


def _pixels(disp, gt, region, occ, conf, thresholds, d1, gt_min, conf_min, occ_min):
    """every per-pixel quantity of the header for one pair of (H, W) float32 arrays"""
    disp, gt = np.asarray(disp, dtype=F), np.asarray(gt, dtype=F)
    assert disp.shape == gt.shape and disp.ndim == 2 and len(thresholds) <= MAX_THR
    with np.errstate(all="ignore"):
        in_region = np.ones(gt.shape, bool) if region is None else np.asarray(region) != 0
        evaluated = in_region & np.isfinite(gt) & (gt > F(gt_min))
        e = disp - gt                                                 # float32
        a = np.abs(e)
        finite = np.isfinite(disp)
        q = np.rint(np.minimum(a, F(1024)) * F(65536))                # float32, exact scaling, half to even
        s = np.rint(np.minimum(e * e, F(1048576)) * F(4096))
        bad = [~finite | (a > F(t)) for t in thresholds]
        d1_bad = ~finite | ((a > F(d1[0])) & (a > F(d1[1]) * np.abs(gt)))
        h = a * F(64)
        hbin = np.where(h >= F(1024), 1024, np.floor(np.where(h >= F(1024), F(0), h))).astype(np.int64)
        if conf is None:
            kept, cbin = np.zeros(gt.shape, bool), None
        else:
            conf, occ = np.asarray(conf, dtype=F), np.asarray(occ, dtype=F)
            kept = (conf > F(conf_min)) & (occ > F(occ_min))
            c = conf * F(64)
            cbin = np.where(~(c >= F(0)), 0, np.where(c >= F(63), 63, np.floor(np.where((c >= F(0)) & (c < F(63)), c, F(0))))).astype(np.int64)
    return dict(in_region=in_region, evaluated=evaluated, finite=finite, e=e, a=a, q=q, s=s, bad=bad, d1=d1_bad, hbin=hbin, kept=kept, cbin=cbin)


def _isum(x, m):
    """exact integer sum of the float32 integers x over mask m"""
    return int(x[m].astype(np.float64).astype(np.uint64).sum(dtype=np.uint64)) if m.any() else 0


def _block(p, sel):
    ev = p["evaluated"] & sel
    out = [0] * BLOCK_WORDS
    out[N_REGION] = int((p["in_region"] & sel).sum())
    out[N_EVAL] = int(ev.sum())
    out[N_NONFINITE] = int((ev & ~p["finite"]).sum())
    out[SUM_ABS_Q] = _isum(p["q"], ev & p["finite"])
    out[SUM_SQ_Q] = _isum(p["s"], ev & p["finite"])
    out[D1_BAD] = int((ev & p["d1"]).sum())
    for t, b in enumerate(p["bad"]):
        out[BAD + t] = int((ev & b).sum())
    return out


def stats(disp, gt, region=None, occ=None, conf=None, thresholds=(0.5, 1.0, 2.0, 4.0), d1=(3.0, 0.05), gt_min=0.0, conf_min=0.1, occ_min=0.5):
    """the stat block of one pair as a list of WORDS Python integers; disp / occ / conf are the CROPPED maps"""
    assert (occ is None) == (conf is None)
    p = _pixels(disp, gt, region, occ, conf, thresholds, d1, gt_min, conf_min, occ_min)
    words = [0] * WORDS
    words[ALL:ALL + BLOCK_WORDS] = _block(p, np.ones(p["evaluated"].shape, bool))
    summed = p["evaluated"] & p["finite"]
    words[HIST:HIST + HIST_BINS] = [int(v) for v in np.bincount(p["hbin"][summed], minlength=HIST_BINS)]
    if conf is not None:
        words[KEPT:KEPT + BLOCK_WORDS] = _block(p, p["kept"])
        for c in range(CONF_BINS):
            m = p["evaluated"] & (p["cbin"] == c)
            row = CONF + c * CONF_ROW_WORDS
            words[row + CONF_COUNT] = int(m.sum())
            words[row + CONF_SUM_ABS_Q] = _isum(p["q"], m & p["finite"])
            for t, b in enumerate(p["bad"]):
                words[row + CONF_BAD + t] = int((m & b).sum())
    return words


def textbook(disp, gt, region=None, occ=None, conf=None, kept=False, thresholds=(0.5, 1.0, 2.0, 4.0), gt_min=0.0, conf_min=0.1, occ_min=0.5):
    """float64 means over the same pixels: the error of a pixel is the float32 difference the header defines, everything after it is float64
    (no fixed point, no clip).  -> dict(n, epe, rmse, max_sq, bad={t: share})"""
    p = _pixels(disp, gt, region, occ, conf, thresholds, (3.0, 0.05), gt_min, conf_min, occ_min)
    ev = p["evaluated"] & (p["kept"] if kept else True)
    m = ev & p["finite"]
    e = p["e"][m].astype(np.float64)
    n = int(ev.sum())
    return dict(n=n, n_finite=int(m.sum()), epe=float(np.abs(e).mean()) if e.size else float("nan"),
                rmse=float(np.sqrt((e * e).mean())) if e.size else float("nan"), max_sq=float((e * e).max()) if e.size else 0.0,
                bad={float(t): (float((ev & b).sum()) / n if n else float("nan")) for t, b in zip(thresholds, p["bad"])})
