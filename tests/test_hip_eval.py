"""K18 on the GPU (include/s2m2_hip.h: s2m2_disp_eval; s2m2_amd/evaluate.py) against the numpy oracle of tests/eval_oracle.py -- never against the
code under test.  Every comparison is EXACT INTEGER EQUALITY OF THE WHOLE STAT BLOCK: oracle and kernel evaluate the same correctly rounded
fp32 chain (one subtraction, one product, comparisons, exact power-of-two scalings; the library is built with -fno-fast-math), so knife edges
are not avoided but put in on purpose (eval_oracle.draw: predictions exactly a threshold above an integer ground truth)."""
import json
import math
import subprocess

import numpy as np
import pytest
import torch

import eval_oracle as EO
from s2m2_amd import evaluate as EV

pytestmark = pytest.mark.gpu

F = np.float32
INF = float("inf")


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _oracle(d, H, W, **kw):
    """the oracle blocks of every pair of the drawn (or hand-made) arrays d: padded maps cropped on the host, then the rules"""
    out = []
    for b in range(d["disp"].shape[0]):
        m = {k: (EO.crop(d[k][b, 0], H, W) if d.get(k) is not None else None) for k in ("disp", "occ", "conf")}
        region = d["region"][b, 0] if d.get("region") is not None else None
        out.append(EO.stats(m["disp"], d["gt"][b, 0], region, m["occ"], m["conf"], **kw))
    return out


def _device(d, **kw):
    H, W = d["gt"].shape[-2:]
    if "d1" in kw:
        kw = dict(kw, d1=tuple(kw["d1"]))
    st = EV.evaluate(_cuda(d["disp"]), _cuda(d["gt"]), region=_cuda(d.get("region")), occ=_cuda(d.get("occ")), conf=_cuda(d.get("conf")), **kw)
    torch.cuda.synchronize()
    return st


def _check(d, **kw):
    H, W = d["gt"].shape[-2:]
    st = _device(d, **kw)
    got, want = st.words.cpu().tolist(), _oracle(d, H, W, **kw)
    for b, (g, w) in enumerate(zip(got, want)):
        if g != w:
            diff = [(i, g[i], w[i]) for i in range(EO.WORDS) if g[i] != w[i]]
            raise AssertionError(f"pair {b}: {len(diff)} words differ, first (word, device, oracle): {diff[:8]}")
    return st, want


def test_less_than_one_wave(hip):
    """5x7, B = 1, no padding: tail lanes, one tile"""
    _, want = _check(EO.draw(1, 5, 7, 5, 7, 1))
    assert want[0][EO.N_REGION] > 0


@pytest.mark.parametrize("H,W", [(64, 96), (61, 93), (63, 96)])
def test_crop_offsets_under_aligned_maps(hip, H, W):
    """64x96 maps: crop offsets 0 / 1, W % 4 != 0, gt rows that start on every alignment"""
    _, want = _check(EO.draw(2, 64, 96, H, W, 10 + H))
    assert want[0][EO.N_EVAL] > 1000 and want[0][EO.KEPT + EO.N_EVAL] > 100 and want[0][EO.HIST + 1024] > 0


def test_scalar_load_paths(hip):
    """Wp = 70 (rows are not 16-byte multiples), and 16-byte-row maps / gt / region passed as views that start one element into their
    allocation (misaligned bases)"""
    _check(EO.draw(1, 66, 70, 63, 67, 21))
    d = EO.draw(1, 64, 96, 64, 96, 22)
    H, W = 64, 96

    def shifted(a):
        buf = torch.zeros(a.size + 1, dtype=torch.from_numpy(a).dtype, device="cuda")
        buf[1:] = torch.from_numpy(a).reshape(-1).cuda()
        v = buf[1:].view(a.shape)
        assert v.data_ptr() % (4 * a.itemsize) != 0 and v.is_contiguous()
        return v

    want = _oracle(d, H, W)
    for which in (("disp",), ("occ", "conf"), ("gt", "region"), ("disp", "occ", "conf", "gt", "region")):
        t = {k: (shifted(d[k]) if k in which else _cuda(d[k])) for k in d}
        st = EV.evaluate(t["disp"], t["gt"], region=t["region"], occ=t["occ"], conf=t["conf"])
        torch.cuda.synchronize()
        assert st.words.cpu().tolist() == want, which


def test_many_tiles_partial_last_tile_and_an_empty_pair(hip):
    """a pair taller than three tiles with a partial last tile, B = 2 with different gt / region per pair; pair 1 has no valid gt at all"""
    W = 200
    rows = hip.eval_tile_rows(1000, W)
    H = 3 * rows + max(1, rows // 3)
    assert hip.eval_tile_rows(H, W) == rows and -(-H // rows) == 4 and H % rows != 0
    d = EO.draw(2, H + 2, W + 8, H, W, 31)
    d["gt"][1] = np.inf
    st, want = _check(d)
    assert want[0][EO.N_EVAL] > 0.5 * H * W and want[1][EO.N_REGION] > 0
    assert not any(want[1][EO.N_EVAL:EO.KEPT]) and not any(want[1][EO.KEPT + EO.N_EVAL:])
    # the empty pair: counts 0; the ratios are 0 / 0 = NaN as documented, never an exception
    assert int(st.count()[1]) == 0 and int(st.nonfinite()[1]) == 0 and int(st.region()[1]) == want[1][EO.N_REGION]
    for v in (st.epe(), st.rmse(), st.bad(1.0), st.d1(), st.density(), st.quantile(0.5), st.epe(True)):
        assert math.isnan(float(v[1])) and not math.isnan(float(v[0]))
    assert st.summary(1)["n_eval"] == 0


def test_rows_wider_than_one_flush_of_the_packed_counters(hip):
    """the kernel counts in 7-bit fields per thread and empties them every 31 steps of 1024 pixels: rows of 40 000 pixels take 40 steps.  Drawn
    maps, then the fullest a field can get: every pixel bad at all eight thresholds (the top field), and every prediction not finite"""
    thr = (0.125, 0.25, 0.5, 1.0, 2.0, 3.0, 4.0, 8.0)
    H, W = 2, 40000
    assert hip.eval_tile_rows(H, W) == 1
    _check(EO.draw(1, H, W, H, W, 60), thresholds=thr)
    gt = np.full((1, 1, H, W), 50.0, dtype=F)
    one = np.ones_like(gt)
    _, want = _check(dict(disp=gt + F(9), occ=one, conf=one, gt=gt, region=None), thresholds=thr)
    assert want[0][EO.BAD:EO.BAD + 8] == [H * W] * 8 and want[0][EO.KEPT + EO.BAD + 7] == H * W and want[0][EO.D1_BAD] == H * W
    _, want = _check(dict(disp=np.full_like(gt, np.nan), occ=one, conf=one, gt=gt, region=None), thresholds=thr[:3])
    assert want[0][EO.N_NONFINITE] == H * W and want[0][EO.BAD:EO.BAD + 8] == [H * W] * 3 + [0] * 5 and want[0][EO.SUM_ABS_Q] == 0


def test_threshold_ties(hip):
    """prediction = integer gt + thr exactly is not bad, one ulp above is; the same for d1_abs, for d1_rel * |gt| with a power-of-two gt, and
    for conf == conf_min / occ == occ_min (not kept)"""
    thr = (0.5, 1.0, 2.0, 4.0)
    H, W = 4, 16
    gt = np.full((1, 1, H, W), 64.0, dtype=F)
    disp = gt.copy()
    conf, occ = np.full_like(gt, 0.75), np.full_like(gt, 0.75)
    up = lambda x: np.nextafter(F(x), F(np.inf))
    for i, t in enumerate(thr):                                   # row 0: at and just above every threshold
        disp[0, 0, 0, 2 * i], disp[0, 0, 0, 2 * i + 1] = F(64) + F(t), up(F(64) + F(t))
    disp[0, 0, 0, 8], disp[0, 0, 0, 9] = F(64) - F(1.0), np.nextafter(F(63), F(-np.inf))            # the same below gt
    disp[0, 0, 1, 0], disp[0, 0, 1, 1] = F(64) + F(3), up(F(64) + F(3))                           # d1_abs = 3 with d1_rel * 64 = 2
    gt[0, 0, 1, 2:4] = 128.0                                                                     # d1_rel * 128 = 4 > d1_abs
    disp[0, 0, 1, 2], disp[0, 0, 1, 3] = F(128) + F(4), up(F(128) + F(4))
    conf[0, 0, 2, 0], occ[0, 0, 2, 1] = F(0.25), F(0.5)                                           # exactly the minima: not kept
    conf[0, 0, 2, 2], occ[0, 0, 2, 3] = up(0.25), up(0.5)                                         # one ulp above: kept
    d = dict(disp=disp, occ=occ, conf=conf, gt=gt, region=None)
    kw = dict(thresholds=thr, d1=(3.0, 0.03125), conf_min=0.25, occ_min=0.5)
    _, want = _check(d, **kw)
    w = want[0]
    # what the oracle must have said for the ties (the kernel equals it): per threshold the pixels strictly above it
    assert w[EO.BAD:EO.BAD + 4] == [1 + 6 + 2 + 4, 1 + 4 + 1 + 4, 1 + 2 + 4, 1 + 1]
    assert w[EO.D1_BAD] == 2 + 2                                    # row 0: 68 and up(68) (4 > 3 and > 2); row 1: up(67), up(132)
    assert w[EO.KEPT + EO.N_EVAL] == H * W - 2 and w[EO.N_EVAL] == H * W


def test_clip_overflow_and_nonfinite_predictions(hip):
    H, W = 48, 96
    g = np.random.default_rng(3)
    gt = (g.random((1, 1, H, W), dtype=F) * F(100) + F(1)).astype(F)
    disp = (gt + F(1030) + g.random((1, 1, H, W), dtype=F) * F(3000)).astype(F)           # 1030: the rounding of the sum stays above 1024
    disp[0, 0, ::2] = gt[0, 0, ::2] - F(1030)
    disp[0, 0, 5, 5], disp[0, 0, 6, 6] = F(3e38), F(-3e38)               # finite, the squared error overflows fp32
    conf, occ = np.full_like(gt, 0.9), np.full_like(gt, 0.9)
    d = dict(disp=disp, occ=occ, conf=conf, gt=gt, region=None)
    _, want = _check(d)
    n = H * W
    assert want[0][EO.N_EVAL] == n and want[0][EO.SUM_ABS_Q] == n << 26 and want[0][EO.SUM_SQ_Q] == n << 32          # beyond any 32-bit sum
    assert want[0][EO.HIST + 1024] == n and want[0][EO.KEPT + EO.SUM_SQ_Q] == n << 32
    assert want[0][EO.CONF + 57 * 10 + EO.CONF_SUM_ABS_Q] == n << 26
    # inf, -inf and NaN predictions scattered over the drawn maps: counted, bad everywhere, in no sum and no bin
    d = EO.draw(1, 48, 96, 48, 96, 4)
    flat = d["disp"].reshape(-1)
    flat[g.choice(flat.size, 300, replace=False)] = np.tile(np.array([np.inf, -np.inf, np.nan], dtype=F), 100)
    clean = EO.draw(1, 48, 96, 48, 96, 4)
    _, want = _check(d)
    ref = _oracle(clean, 48, 96)[0]
    nf = want[0][EO.N_NONFINITE]
    assert 100 < nf <= 300 and want[0][EO.N_EVAL] == ref[EO.N_EVAL]
    assert sum(want[0][EO.HIST:EO.CONF]) == ref[EO.N_EVAL] - nf and want[0][EO.SUM_ABS_Q] < ref[EO.SUM_ABS_Q]
    assert all(want[0][EO.BAD + t] >= nf for t in range(4)) and want[0][EO.D1_BAD] >= nf


def test_confidence_binning(hip):
    """1.0, 63/64, 1/64 - ulp, -0.1, 1.5 and NaN land in bins 63, 63, 0, 0, 63 and 0"""
    vals = np.array([1.0, 63.0 / 64.0, np.nextafter(F(1.0 / 64.0), F(0)), -0.1, 1.5, np.nan, 1.0 / 64.0, 0.5], dtype=F)
    H, W = 3, 8
    conf = np.tile(vals, (1, 1, H, 1)).astype(F)
    gt = np.full((1, 1, H, W), 10.0, dtype=F)
    disp = gt + F(0.75)
    d = dict(disp=disp.astype(F), occ=np.ones_like(gt), conf=conf, gt=gt, region=None)
    _, want = _check(d)
    count = [want[0][EO.CONF + c * 10] for c in range(64)]
    assert count[63] == 3 * H and count[0] == 3 * H and count[1] == H and count[32] == H and sum(count) == H * W
    assert want[0][EO.CONF + 63 * 10 + EO.CONF_BAD] == 3 * H and want[0][EO.CONF + 63 * 10 + EO.CONF_BAD + 1] == 0


@pytest.mark.parametrize("thresholds", [(), (1.0,), (0.125, 0.25, 0.5, 1.0, 2.0, 3.0, 4.0, 8.0)], ids=["nthr0", "nthr1", "nthr8"])
def test_threshold_counts(hip, thresholds):
    _, want = _check(EO.draw(1, 32, 64, 30, 61, 40), thresholds=thresholds)
    assert all(want[0][EO.BAD + t] > 0 for t in range(len(thresholds))) and not any(want[0][EO.BAD + len(thresholds):EO.KEPT])


def test_optional_operands(hip):
    d = EO.draw(2, 32, 64, 30, 61, 41)
    _, want = _check(dict(d, occ=None, conf=None))                   # KEPT and CONF all zero
    assert not any(want[0][EO.KEPT:EO.HIST]) and not any(want[0][EO.CONF:]) and want[0][EO.N_EVAL] > 0
    _, want = _check(dict(d, region=None))
    assert want[0][EO.N_REGION] == 30 * 61
    _, neg = _check(d, gt_min=-INF)                                  # every finite gt, the negative ones included
    _, pos = _check(d)
    assert neg[0][EO.N_EVAL] > pos[0][EO.N_EVAL]
    with pytest.raises(ValueError):
        EV.evaluate(_cuda(d["disp"]), _cuda(d["gt"]), occ=_cuda(d["occ"]))            # occ without conf: the binding's own check or the library's


def test_prefilled_buffers_repeat_and_graph_replay(hip):
    d = EO.draw(2, 64, 96, 61, 93, 50)
    want = _oracle(d, 61, 93)
    t = {k: _cuda(v) for k, v in d.items()}
    need = hip.eval_workspace_bytes(2, 61, 93)
    kw = dict(region=t["region"], occ=t["occ"], conf=t["conf"])

    def run(ws, stats):
        hip.disp_eval(t["disp"], t["gt"], stats, ws, **kw)

    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    stats = torch.full((2, hip.EVAL_WORDS), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    run(ws, stats)
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == want
    again = torch.zeros_like(stats)
    run(ws, again)                                                   # the workspace now holds the partial blocks of the first call
    torch.cuda.synchronize()
    assert torch.equal(again, stats)
    # the public function with a caller's workspace
    st = EV.evaluate(t["disp"], t["gt"], workspace=torch.zeros(need, dtype=torch.uint8, device="cuda"), **kw)
    assert torch.equal(st.words, stats)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(ws, again)                                               # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    captured = torch.zeros_like(stats)
    with torch.cuda.graph(graph):
        run(ws, captured)
    for fill in (0x11, 0x77):
        captured.fill_(fill)
        ws.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, stats)


def _s_model():
    from s2m2_amd.model import S2M2
    from s2m2_amd.spec import MODEL_CONFIGS
    from s2m2_amd.weights import seeded_state_dict
    C, ntr = MODEL_CONFIGS["S"]
    m = S2M2(C, 1, ntr, use_positivity=True, refine_iter=3)
    m.load_state_dict(seeded_state_dict(C, 1, ntr, 0), strict=True)
    return m.cuda().eval()


def _gt_for(disp_crop, seed):
    """a ground truth for a model output: the output plus noise of mixed scale, some pixels invalid, and a region"""
    g = np.random.default_rng(seed)
    shape = disp_crop.shape
    noise = (F(10) ** (g.random(shape, dtype=F) * F(3) - F(2))) * g.choice(np.array([-1, 1], dtype=F), shape)
    gt = (disp_crop + noise).astype(F)
    gt[g.random(shape) < 0.1] = np.inf
    region = (g.random(shape) >= 0.2).astype(np.uint8)
    return gt, region


def test_evaluate_behind_a_real_forward(hip):
    """S model, seeded weights, a 60x90 pair padded to 64x96: evaluate() on the padded maps against the oracle on the cropped ones, and
    EvalStats.summary() against the float64 textbook within the bounds of tests/test_eval_cpu.py"""
    from s2m2_amd import utils
    from s2m2_amd.weights import synthetic_pair
    H, W = 60, 90
    m = _s_model()
    left, right = synthetic_pair(H, W, 1, 8, 3)
    lp, rp = utils.image_pad(left.to(torch.uint8).cuda(), 32), utils.image_pad(right.to(torch.uint8).cuda(), 32)
    with torch.autocast("cuda", dtype=torch.float16):
        disp, occ, conf = (t.float().contiguous() for t in m(lp, rp))
    torch.cuda.synchronize()
    assert tuple(disp.shape) == (1, 1, 64, 96)
    host = {k: t.cpu().numpy() for k, t in (("disp", disp), ("occ", occ), ("conf", conf))}
    gt, region = _gt_for(EO.crop(host["disp"], H, W), 8)
    st = utils.evaluate(disp, _cuda(gt), region=_cuda(region), occ=occ, conf=conf, gt_min=-INF)
    torch.cuda.synchronize()
    want = _oracle(dict(host, gt=gt, region=region), H, W, gt_min=-INF)
    assert st.words.cpu().tolist() == want
    s = st.summary()
    for kept, got in ((False, s), (True, s["kept"])):
        tb = EO.textbook(EO.crop(host["disp"][0, 0], H, W), gt[0, 0], region[0, 0], EO.crop(host["occ"][0, 0], H, W), EO.crop(host["conf"][0, 0], H, W),
                         kept=kept, gt_min=-INF)
        print(f"[eval e2e] kept={kept}: n {tb['n']}  epe {got['epe']:.6f} px (float64 {tb['epe']:.6f})  rmse {got['rmse']:.6f} (float64 {tb['rmse']:.6f})")
        assert got["n_eval"] == tb["n"] and (kept or tb["n"] > 3000)
        if tb["n_finite"] == 0:
            continue
        assert tb["max_sq"] < 1024.0 ** 2
        assert abs(got["epe"] - tb["epe"]) <= 2.0 ** -17
        bound = 2.0 ** -13 + 2.0 ** -24 * tb["max_sq"]
        assert abs(got["rmse"] - tb["rmse"]) <= bound / (got["rmse"] + tb["rmse"])
        for t in (0.5, 1.0, 2.0, 4.0):
            assert got[f"bad_{t:g}"] == tb["bad"][t]


def test_runner_writes_the_metrics(hip, tmp_path):
    """s2m2_run_engine --gt / --gt-region / --metrics in a fresh process: the raw words of the JSON against evaluate() on the maps the same run
    wrote with --out"""
    from s2m2_amd.build import RUNNER
    from s2m2_amd.export import export_engine
    from s2m2_amd.weights import synthetic_pair
    H, W = 64, 96
    m = _s_model()
    path = str(tmp_path / "s_64x96.s2m2")
    export_engine(m, path, H, W)
    left, right = synthetic_pair(H, W, 1, 8, 11)
    (tmp_path / "left.f32").write_bytes(left.contiguous().numpy().astype("<f4").tobytes())
    (tmp_path / "right.f32").write_bytes(right.contiguous().numpy().astype("<f4").tobytes())
    base = [RUNNER, path, str(tmp_path / "left.f32"), str(tmp_path / "right.f32")]
    out = tmp_path / "out"
    out.mkdir()
    # a first run for the maps, from which the ground truth is made
    p = subprocess.run(base + ["--out", str(out)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr
    maps = [np.fromfile(out / f"{n}.f32", dtype="<f4").reshape(1, 1, H, W) for n in ("disp", "occ", "conf")]
    gt, region = _gt_for(maps[0], 12)
    EV.write_pfm(str(tmp_path / "gt.pfm"), gt[0, 0])
    (tmp_path / "r.u8").write_bytes(region.tobytes())
    thr = (0.5, 1.0, 3.0)
    p = subprocess.run(base + ["--out", str(out), "--gt", str(tmp_path / "gt.pfm"), "--gt-region", str(tmp_path / "r.u8"), "--gt-min", "-inf",
                               "--thresholds", "0.5,1,3", "--metrics", str(tmp_path / "m.json"), "--repeat", "2"],
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr
    assert "ms_per_pair" in p.stdout and "eval_us_per_pair" in p.stdout
    again = [np.fromfile(out / f"{n}.f32", dtype="<f4").reshape(1, 1, H, W) for n in ("disp", "occ", "conf")]
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(maps, again))
    st = EV.evaluate(_cuda(again[0]), _cuda(gt), region=_cuda(region), occ=_cuda(again[1]), conf=_cuda(again[2]), thresholds=thr, gt_min=-INF)
    torch.cuda.synchronize()
    js = json.loads((tmp_path / "m.json").read_text())
    assert js["thresholds"] == list(thr) and len(js["pairs"]) == 1
    assert js["pairs"][0]["words"] == st.words[0].cpu().tolist()
    assert js["pairs"][0]["words"] == _oracle(dict(disp=again[0], occ=again[1], conf=again[2], gt=gt, region=region), H, W, thresholds=thr, gt_min=-INF)[0]
    s = st.summary()
    assert js["pairs"][0]["n_eval"] == s["n_eval"] > 3000
    for key in ("epe", "rmse", "d1", "bad_0.5", "bad_1", "bad_3", "density", "a50", "a99"):
        assert math.isclose(js["pairs"][0][key], s[key], rel_tol=1e-12), key
    assert math.isclose(js["pairs"][0]["kept"]["epe"], s["kept"]["epe"], rel_tol=1e-12)
    # option errors are usage errors; a malformed ground truth fails before the engine is loaded
    q = subprocess.run(base + ["--gt", str(tmp_path / "gt.pfm")], capture_output=True, text=True, timeout=60)
    assert q.returncode != 0 and "--gt and --metrics come together" in q.stderr
    (tmp_path / "short.pfm").write_bytes((tmp_path / "gt.pfm").read_bytes()[:-8])
    q = subprocess.run([RUNNER, str(tmp_path / "missing.s2m2"), base[2], base[3], "--gt", str(tmp_path / "short.pfm"), "--metrics", str(tmp_path / "x.json")],
                       capture_output=True, text=True, timeout=60)
    assert q.returncode != 0 and "--gt" in q.stderr and "cannot load the engine" not in q.stderr
