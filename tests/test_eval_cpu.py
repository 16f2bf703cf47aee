"""CPU-side checks of the evaluation stage (K18: include/s2m2_hip.h s2m2_disp_eval, s2m2_amd/evaluate.py): the numpy oracle against a float64
textbook, the derivations of EvalStats on CPU tensors, the PFM reader / writer, and the C boundary (descriptor layout, constants, every
validation path -- all of which return before any device call, there is no GPU here)."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import eval_oracle as EO
from s2m2_amd import evaluate as EV
from s2m2_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    from s2m2_amd.build import build
    build(verbose=False)
    return hip.load()


@pytest.fixture(scope="module")
def case():
    """one drawn pair (61x93 inside 64x96) and its oracle block, shared and left unchanged"""
    d = EO.draw(1, 64, 96, 61, 93, 5)
    maps = {k: EO.crop(d[k][0, 0], 61, 93) for k in ("disp", "occ", "conf")}
    words = EO.stats(maps["disp"], d["gt"][0, 0], d["region"][0, 0], maps["occ"], maps["conf"])
    return d, maps, words


# ------------------------------------------------------------------------------------------------ oracle vs textbook

def test_oracle_layout_constants():
    assert EO.WORDS == 1693 and EO.KEPT == EO.ALL + EO.BLOCK_WORDS and EO.HIST == EO.KEPT + EO.BLOCK_WORDS and EO.CONF == EO.HIST + EO.HIST_BINS
    for name in ("N_REGION", "N_EVAL", "N_NONFINITE", "SUM_ABS_Q", "SUM_SQ_Q", "D1_BAD", "BAD", "BLOCK_WORDS", "CONF_COUNT", "CONF_SUM_ABS_Q", "CONF_BAD",
                 "CONF_ROW_WORDS", "ALL", "KEPT", "HIST", "CONF", "WORDS", "MAX_THR", "HIST_BINS", "CONF_BINS"):
        assert getattr(EO, name) == getattr(hip, "EVAL_" + name), name


@pytest.mark.parametrize("kept", [False, True])
def test_oracle_against_the_float64_textbook(case, kept):
    """every q is within 2^-17 px of |e| below the clip (one rounding to a multiple of 2^-16), so the fixed-point EPE is within 2^-17 px of the
    float64 mean.  Every s is within 2^-13 px^2 of the float32 product e * e (one rounding to a multiple of 2^-12), which is within
    2^-24 * e^2 of the exact square: the mean squares differ by at most 2^-13 + 2^-24 * max e^2, and |sqrt x - sqrt y| = |x - y| / (sqrt x +
    sqrt y).  The counts are exact."""
    d, maps, words = case
    tb = EO.textbook(maps["disp"], d["gt"][0, 0], d["region"][0, 0], maps["occ"], maps["conf"], kept=kept)
    blk = words[EO.KEPT:EO.KEPT + EO.BLOCK_WORDS] if kept else words[EO.ALL:EO.ALL + EO.BLOCK_WORDS]
    assert tb["max_sq"] < 1024.0 ** 2 and tb["n"] > 500
    assert blk[EO.N_EVAL] == tb["n"] and blk[EO.N_EVAL] - blk[EO.N_NONFINITE] == tb["n_finite"]
    epe = blk[EO.SUM_ABS_Q] / 65536.0 / tb["n_finite"]
    assert abs(epe - tb["epe"]) <= 2.0 ** -17
    mse = blk[EO.SUM_SQ_Q] / 4096.0 / tb["n_finite"]
    bound = 2.0 ** -13 + 2.0 ** -24 * tb["max_sq"]
    assert abs(mse - tb["rmse"] ** 2) <= bound
    assert abs(math.sqrt(mse) - tb["rmse"]) <= bound / (math.sqrt(mse) + tb["rmse"])
    for i, t in enumerate((0.5, 1.0, 2.0, 4.0)):
        assert blk[EO.BAD + i] == round(tb["bad"][t] * tb["n"])
    for i in range(4, 8):
        assert blk[EO.BAD + i] == 0


def test_oracle_on_hand_computed_pixels():
    """six pixels: errors 0.25, exactly 0.5 (a tie: not bad), 3.5 with gt 100 (d1: 3.5 > 3 but not > 5), 3.5 with gt 10 (d1), a NaN prediction,
    and an invalid gt (inf)"""
    gt = np.array([[10, 20, 100, 10, 10, np.inf]], dtype=np.float32)
    disp = np.array([[10.25, 20.5, 103.5, 13.5, np.nan, 7.0]], dtype=np.float32)
    conf = np.array([[0.9, 0.05, 0.9, 0.9, 0.9, 0.9]], dtype=np.float32)
    occ = np.array([[0.9, 0.9, 0.9, 0.4, 0.9, 0.9]], dtype=np.float32)
    w = EO.stats(disp, gt, None, occ, conf)
    assert w[EO.ALL:EO.ALL + 6] == [6, 5, 1, int((0.25 + 0.5 + 3.5 + 3.5) * 65536), int((0.0625 + 0.25 + 12.25 + 12.25) * 4096), 2]
    assert w[EO.ALL + EO.BAD:EO.ALL + EO.BAD + 8] == [3, 3, 3, 1, 0, 0, 0, 0]
    assert w[EO.KEPT:EO.KEPT + 6] == [4, 3, 1, int((0.25 + 3.5) * 65536), int((0.0625 + 12.25) * 4096), 1]
    assert w[EO.KEPT + EO.BAD:EO.KEPT + EO.BAD + 8] == [2, 2, 2, 1, 0, 0, 0, 0]
    hist = w[EO.HIST:EO.HIST + EO.HIST_BINS]
    assert sum(hist) == 4 and hist[16] == 1 and hist[32] == 1 and hist[224] == 2
    row = lambda c: w[EO.CONF + c * 10:EO.CONF + c * 10 + 10]
    assert row(57) == [4, int((0.25 + 3.5 + 3.5) * 65536), 3, 3, 3, 1, 0, 0, 0, 0]         # 0.9 * 64 = 57.6
    assert row(3) == [1, int(0.5 * 65536), 0, 0, 0, 0, 0, 0, 0, 0]                          # 0.05 * 64 = 3.2
    assert sum(w[EO.CONF:]) == sum(row(57)) + sum(row(3))
    # without occ / conf: KEPT and CONF are zero, the rest is unchanged
    n = EO.stats(disp, gt)
    assert n[:EO.KEPT] == w[:EO.KEPT] and n[EO.HIST:EO.CONF] == hist and not any(n[EO.KEPT:EO.HIST]) and not any(n[EO.CONF:])


# ------------------------------------------------------------------------------------------------ EvalStats on CPU tensors

def _stats(words, thresholds=(0.5, 1.0, 2.0, 4.0)):
    return EV.EvalStats(torch.tensor([words] if isinstance(words[0], int) else words, dtype=torch.int64), thresholds)


def test_evalstats_derivations_on_cpu_tensors(case):
    d, maps, words = case
    st = _stats(words)
    for kept in (False, True):
        tb = EO.textbook(maps["disp"], d["gt"][0, 0], d["region"][0, 0], maps["occ"], maps["conf"], kept=kept)
        blk = words[EO.KEPT:EO.KEPT + 14] if kept else words[:14]
        assert int(st.count(kept)[0]) == tb["n"] and int(st.region(kept)[0]) == blk[EO.N_REGION] and int(st.nonfinite(kept)[0]) == 0
        assert float(st.epe(kept)[0]) == blk[EO.SUM_ABS_Q] / 65536.0 / tb["n_finite"]
        assert float(st.rmse(kept)[0]) == math.sqrt(blk[EO.SUM_SQ_Q] / 4096.0 / tb["n_finite"])
        assert abs(float(st.epe(kept)[0]) - tb["epe"]) <= 2.0 ** -17
        for t in (0.5, 1.0, 2.0, 4.0):
            assert float(st.bad(t, kept)[0]) == tb["bad"][t]
        assert float(st.d1(kept)[0]) == blk[EO.D1_BAD] / tb["n"]
    assert float(st.density()[0]) == words[EO.KEPT + EO.N_EVAL] / words[EO.N_EVAL]
    with pytest.raises(KeyError):
        st.bad(3.0)
    # quantiles: the definition, spelled out on the histogram
    hist = words[EO.HIST:EO.HIST + EO.HIST_BINS]
    n = sum(hist)
    for p in (0.5, 0.9, 0.95, 0.99, 1.0):
        cum, want = 0, None
        for i, h in enumerate(hist):
            cum += h
            if cum >= p * n:
                want = INF if i == 1024 else (i + 1) / 64.0
                break
        assert float(st.quantile(p)[0]) == want, p
    assert float(st.quantile(0.5)[0]) < float(st.quantile(0.99)[0])
    # by_confidence: suffix sums of the table
    by = st.by_confidence()
    rows = [words[EO.CONF + c * 10:EO.CONF + c * 10 + 10] for c in range(64)]
    for k in (0, 1, 17, 63):
        cnt = sum(r[0] for r in rows[k:])
        assert float(by["density"][0, k]) == cnt / words[EO.N_EVAL]
        assert float(by["epe"][0, k]) == sum(r[1] for r in rows[k:]) / 65536.0 / cnt
        assert float(by["bad"][1.0][0, k]) == sum(r[3] for r in rows[k:]) / cnt
    assert float(by["density"][0, 0]) == 1.0 and float(by["epe"][0, 0]) == float(st.epe()[0])
    assert tuple(by["density"].shape) == (1, 64)
    s = st.summary()
    assert s["n_eval"] == words[EO.N_EVAL] and s["epe"] == float(st.epe()[0]) and s["kept"]["bad_1"] == float(st.bad(1.0, True)[0])
    assert s["a50"] == float(st.quantile(0.5)[0]) and s["density"] == float(st.density()[0])


def test_evalstats_add_total_and_empty_blocks(case):
    d, maps, words = case
    other = EO.stats(maps["disp"], d["gt"][0, 0], None, maps["occ"], maps["conf"])
    a, b = _stats(words), _stats(other)
    both = a + b
    assert both.words.tolist() == [[x + y for x, y in zip(words, other)]]
    two = _stats([words, other])
    assert two.total().words.tolist() == both.words.tolist()
    assert float(both.epe()[0]) == (words[EO.SUM_ABS_Q] + other[EO.SUM_ABS_Q]) / 65536.0 / (words[EO.N_EVAL] + other[EO.N_EVAL])
    with pytest.raises(ValueError):
        a + _stats(other, thresholds=(1.0,))
    # a pair without a valid pixel: counts 0, every ratio 0 / 0 = NaN (documented in s2m2_amd/evaluate.py), nothing raises
    empty = _stats([0] * EO.WORDS)
    assert int(empty.count()[0]) == 0 and int(empty.nonfinite()[0]) == 0
    for v in (empty.epe(), empty.rmse(), empty.bad(1.0), empty.d1(), empty.density(), empty.quantile(0.5), empty.by_confidence()["epe"][:, 0]):
        assert math.isnan(float(v[0]))
    assert math.isnan(empty.summary()["kept"]["epe"])
    # the overflow bin is "16 px and more": its upper edge is inf
    w = [0] * EO.WORDS
    w[EO.HIST + 3], w[EO.HIST + 1024] = 1, 3
    assert float(_stats(w).quantile(0.25)[0]) == 4 / 64.0 and float(_stats(w).quantile(0.5)[0]) == INF


def test_all_reduce_is_one_sum_collective(case):
    _, _, words = case

    class Dist:
        class ReduceOp:
            SUM = "sum"
        calls = []

        @classmethod
        def all_reduce(cls, t, op=None, group=None):
            cls.calls.append((tuple(t.shape), t.dtype, op, group))
            t.mul_(2)                                               # two ranks holding the same block

    st = _stats(words).total()
    assert st.all_reduce(Dist, group="g") is st
    assert Dist.calls == [((1, EO.WORDS), torch.int64, "sum", "g")] and st.words[0].tolist() == [2 * x for x in words]


def test_evaluate_rejects_host_tensors():
    z = torch.zeros(1, 1, 32, 32)
    with pytest.raises(ValueError, match="device tensors"):
        EV.evaluate(z, z)
    from s2m2_amd import utils
    assert utils.evaluate is EV.evaluate


# ------------------------------------------------------------------------------------------------ PFM

@pytest.mark.parametrize("little", [True, False])
def test_pfm_round_trip(tmp_path, little):
    a = np.arange(12, dtype=np.float32).reshape(3, 4) * np.float32(1.25) - np.float32(3)
    a[1, 2], a[2, 0] = np.inf, -0.0
    path = str(tmp_path / "a.pfm")
    EV.write_pfm(path, a, little_endian=little)
    raw = open(path, "rb").read()
    head = raw[:len(raw) - 48].decode().split("\n")
    assert head[0] == "Pf" and head[1] == "4 3" and (float(head[2]) < 0) == little
    # rows are stored bottom to top: the first stored row is the LAST row of the array
    assert np.array_equal(np.frombuffer(raw[-48:], dtype="<f4" if little else ">f4")[:4], a[2])
    back = EV.read_pfm(path)
    assert back.dtype == np.float32 and back.shape == (3, 4) and back.tobytes() == a.tobytes() and np.isinf(back[1, 2])


def test_pfm_errors(tmp_path):
    def bad(name, blob, msg):
        (tmp_path / name).write_bytes(blob)
        with pytest.raises(ValueError, match=msg):
            EV.read_pfm(str(tmp_path / name))
    data = np.zeros(6, dtype="<f4").tobytes()
    bad("colour.pfm", b"PF\n3 2\n-1.0\n" + data * 3, "colour")
    bad("magic.pfm", b"P5\n3 2\n-1.0\n" + data, "not a PFM")
    bad("dims.pfm", b"Pf\n3 two\n-1.0\n" + data, "malformed")
    bad("onedim.pfm", b"Pf\n3\n-1.0\n" + data, "malformed")
    bad("scale.pfm", b"Pf\n3 2\n0\n" + data, "malformed")
    bad("neg.pfm", b"Pf\n-3 2\n-1.0\n" + data, "malformed")
    bad("short.pfm", b"Pf\n3 2\n-1.0\n" + data[:-4], "bytes of data")
    bad("long.pfm", b"Pf\n3 2\n-1.0\n" + data + b"\0\0\0\0", "bytes of data")
    bad("header.pfm", b"Pf\n3 2", "three lines")
    with pytest.raises(ValueError):
        EV.write_pfm(str(tmp_path / "x.pfm"), np.zeros((2, 2, 3), dtype=np.float32))


# ------------------------------------------------------------------------------------------------ the C boundary

def test_symbols_and_version(lib):
    for n in ("s2m2_disp_eval", "s2m2_eval_workspace_bytes", "s2m2_eval_tile_rows"):
        assert hasattr(lib, n) and n in hip.SIGNATURES
    assert lib.s2m2_version() == 800 and hip.ABI_VERSION == 800


def test_eval_desc_and_constants_are_the_header_s(tmp_path):
    """every field of hip.EvalDesc (offset, size) and every S2M2_EVAL_* constant against include/s2m2_hip.h compiled by gcc"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = [f[0] for f in hip.EvalDesc._fields_]
    consts = ["N_REGION", "N_EVAL", "N_NONFINITE", "SUM_ABS_Q", "SUM_SQ_Q", "D1_BAD", "BAD", "BLOCK_WORDS", "CONF_COUNT", "CONF_SUM_ABS_Q", "CONF_BAD",
              "CONF_ROW_WORDS", "ALL", "KEPT", "HIST", "CONF", "WORDS", "MAX_THR", "HIST_BINS", "CONF_BINS"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "s2m2_hip.h"', "int main(void) {", "  s2m2_eval_desc d;",
             '  printf("%zu\\n", sizeof(d));']
    lines += [f'  printf("{n} %zu %zu\\n", offsetof(s2m2_eval_desc, {n}), sizeof(d.{n}));' for n in names]
    lines += [f'  printf("{c} %d\\n", (int)S2M2_EVAL_{c});' for c in consts]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == ctypes.sizeof(hip.EvalDesc)
    for n, line in zip(names, out[1:]):
        name, off, size = line.split()
        f = getattr(hip.EvalDesc, n)
        assert (name, int(off), int(size)) == (n, f.offset, f.size)
    for c, line in zip(consts, out[1 + len(names):]):
        name, val = line.split()
        assert name == c and int(val) == getattr(hip, "EVAL_" + c) == getattr(EO, c), c
    assert hip.EVAL_WORDS == 1693


def _desc(**over):
    """a descriptor that passes validation (the pointers are never dereferenced on the host)"""
    d = hip.EvalDesc()
    d.disp = d.occ = d.conf = d.gt = d.region = d.workspace = d.stats = 4096
    d.B, d.H, d.W, d.Hp, d.Wp, d.nthr = 1, 30, 50, 32, 64, 4
    for i, t in enumerate((0.5, 1.0, 2.0, 4.0)):
        d.thr[i] = t
    d.d1_abs, d.d1_rel, d.gt_min, d.conf_min, d.occ_min = 3.0, 0.05, 0.0, 0.1, 0.5
    for k, v in over.items():
        if k == "thr":
            for i, t in enumerate(v):
                d.thr[i] = t
        else:
            setattr(d, k, v)
    return d


NAN = float("nan")
BAD = [
    (dict(disp=None), b"null pointer"),
    (dict(gt=None), b"null pointer"),
    (dict(stats=None), b"null pointer"),
    (dict(workspace=None), b"null pointer"),
    (dict(occ=None), b"occ and conf come together"),
    (dict(conf=None), b"occ and conf come together"),
    (dict(B=0), b"non-positive extents"),
    (dict(H=0), b"non-positive extents"),
    (dict(W=-3), b"non-positive extents"),
    (dict(Hp=0), b"non-positive extents"),
    (dict(Wp=-1), b"non-positive extents"),
    (dict(H=33), b"larger than the maps"),
    (dict(W=65), b"larger than the maps"),
    (dict(nthr=-1), b"nthr"),
    (dict(nthr=9), b"nthr"),
    (dict(thr=(0.5, 0.5, 2.0, 4.0)), b"strictly increasing"),
    (dict(thr=(1.0, 0.5, 2.0, 4.0)), b"strictly increasing"),
    (dict(thr=(0.0, 0.5, 2.0, 4.0)), b"strictly increasing"),
    (dict(thr=(-1.0, 0.5, 2.0, 4.0)), b"strictly increasing"),
    (dict(thr=(0.5, 1.0, 2.0, NAN)), b"strictly increasing"),
    (dict(thr=(0.5, 1.0, 2.0, INF)), b"strictly increasing"),
    (dict(d1_abs=INF), b"d1_abs and d1_rel must be finite"),
    (dict(d1_rel=NAN), b"d1_abs and d1_rel must be finite"),
    (dict(conf_min=NAN), b"conf_min and occ_min must be finite"),
    (dict(occ_min=-INF), b"conf_min and occ_min must be finite"),
    (dict(gt_min=NAN), b"gt_min is NaN"),
    (dict(workspace=4100), b"8-byte aligned"),
    (dict(gt=4098), b"4-byte aligned"),
]


@pytest.mark.parametrize("over,msg", BAD, ids=[f"{'-'.join(o)}-{i}" for i, (o, _) in enumerate(BAD)])
def test_validation_fails_before_any_device_call(lib, over, msg):
    assert lib.s2m2_disp_eval(ctypes.byref(_desc(**over)), None) != 0
    assert msg in lib.s2m2_last_error(), lib.s2m2_last_error()


def test_null_descriptor_and_plan_recording(lib):
    assert lib.s2m2_disp_eval(None, None) != 0 and b"null descriptor" in lib.s2m2_last_error()
    plan = ctypes.c_void_p()
    assert lib.s2m2_plan_begin(ctypes.byref(plan)) == 0
    try:
        # a descriptor that is valid in every field (gt_min = -inf and no occ / conf / region included) is still refused while a plan records
        assert lib.s2m2_disp_eval(ctypes.byref(_desc(gt_min=-INF, occ=None, conf=None, region=None, nthr=0)), None) != 0
        assert b"not recorded in launch plans" in lib.s2m2_last_error()
        assert lib.s2m2_plan_launches(plan) == 0
    finally:
        lib.s2m2_plan_abort(plan)
        lib.s2m2_plan_destroy(plan)
    header = open(os.path.join(ROOT, "include", "s2m2_hip.h")).read()
    assert "s2m2_disp_eval is NOT recorded" in header
    assert int(re.search(r"#define S2M2_ABI_VERSION (\d+)", header).group(1)) == 800


def test_workspace_size_and_tile_rows(lib):
    for bad in ((0, 4, 4), (1, -1, 4), (1, 4, 0), (70000, 4, 4), (1, 65536, 65536)):
        assert lib.s2m2_eval_workspace_bytes(*bad) == 0
    assert lib.s2m2_eval_tile_rows(0, 4) == 0 and lib.s2m2_eval_tile_rows(4, -1) == 0
    for B, H, W in ((1, 1, 1), (1, 1024, 1216), (3, 2048, 2432), (2, 5000, 7)):
        rows = lib.s2m2_eval_tile_rows(H, W)
        tiles = -(-H // rows)
        assert rows >= 1 and tiles <= 1024
        # one partial block per tile: at least the low halves of every word
        assert lib.s2m2_eval_workspace_bytes(B, H, W) >= B * tiles * 4 * hip.EVAL_WORDS
        assert hip.eval_workspace_bytes(B, H, W) == lib.s2m2_eval_workspace_bytes(B, H, W) and hip.eval_tile_rows(H, W) == rows
    with pytest.raises(ValueError):
        hip.eval_workspace_bytes(0, 1, 1)
