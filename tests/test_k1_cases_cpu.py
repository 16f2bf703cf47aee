"""The cases of tests/test_hip_k1_blocks.py reach the launches they claim, and their comparator has teeth (CPU, no kernel).

1. s2m2_amd/csrc/ln_corr_select.h is plain C++: a small host program prints the plan of every case of tests/k1_cases.py.  Every claimed
   plan must be the planner's, and over the whole list every (token dtype, volume dtype, C) must see its widest block, a wave past the row
   end, more than one chunk on a block of more than two waves (fp32 C = 384 launches two waves at most) and no block of two waves or fewer.
   A change of a threshold fails here: it cannot move the GPU tests back onto two-wave blocks.
2. The float64 reference against a numpy restatement.
3. A torch emulation of K1's arithmetic (fp32 LayerNorm, operands rounded to the token dtype, fp32 product, rounded to the volume dtype)
   goes through the GPU test's own comparator and bounds at every case's width (two image rows: the planner is not involved) -- it must pass
   -- and so does each of seven deliberately wrong variants, which every case it applies to must reject."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import k1_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (1, 2)                             # (B, h) of the emulation runs

PROGRAM = r"""
#include <stdio.h>
#include "s2m2_amd/csrc/ln_corr_select.h"
int main() {
    int B, h, w, pitch, tb, cb, C;
    while (scanf("%d %d %d %d %d %d %d", &B, &h, &w, &pitch, &tb, &cb, &C) == 7) {
        const s2m2::LnCorrShape s = s2m2::ln_corr_shape(tb, cb, C);
        const s2m2::LnCorrPlan p = s2m2::ln_corr_plan(B, h, w, pitch, tb, cb, C);
        printf("%d %d %d %d %d %d %d\n", p.nstrip, p.nw, p.nchunks, p.store_mode, s.nwmax, s.nwgran, s.tpw);
    }
    return 0;
}
"""


def _compiler():
    for cc in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cc)
        if path:
            return path
    raise RuntimeError("no host C++ compiler found (c++, g++, clang++)")


def _pitch(w, cdt, aligned):
    per = 128 // K.BYTES[cdt]
    return (w + per - 1) // per * per if aligned else w


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """(case id, aligned rows) -> (nstrip, nw, nchunks, store mode, NWMAX, NWGRAN, TPW) from one run of the host program"""
    tmp = tmp_path_factory.mktemp("k1plan")
    src, exe = tmp / "plan.cpp", tmp / "plan"
    src.write_text(PROGRAM)
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", "-I", ROOT, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    keys, lines = [], []
    for c in K.all_cases():
        B, h, w = c.dims
        for aligned in (False, True):
            keys.append((c.id, aligned))
            lines.append(f"{B} {h} {w} {_pitch(w, c.cdt, aligned)} {K.BYTES[c.tdt]} {K.BYTES[c.cdt]} {c.C}")
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout
    rows = [tuple(int(v) for v in ln.split()) for ln in out.strip().splitlines()]
    assert len(rows) == len(keys)
    return dict(zip(keys, rows))


def test_header_needs_no_hip():
    text = open(os.path.join(ROOT, "s2m2_amd", "csrc", "ln_corr_select.h")).read()
    assert "hip/" not in text and "common.h" not in text and "#include" not in text


def test_case_list():
    cs = K.all_cases()
    assert len({c.id for c in cs}) == len(cs)
    for shape in "ABCD":                                                # A - D: all 15 configurations in both forms
        assert {(c.tdt, c.cdt, c.C, c.form) for c in cs if c.shape == shape} == {cfg + (f,) for cfg in K.CONFIGS for f in K.FORMS}
    assert len(K.cases(shapes="ABCD")) == 120
    assert {(c.tdt, c.C) for c in K.cases(shapes="E")} == {("float16", 64)}


def test_every_claimed_plan_is_the_planners(planned):
    wrong = []
    for c in K.all_cases():
        B, h, w = c.dims
        tiles = (w + 31) // 32
        for aligned in (False, True):
            nstrip, nw, nchunks, mode, nwmax, nwgran, tpw = planned[(c.id, aligned)]
            got = K.Plan(nstrip, nw, nchunks, nstrip * nw - tiles, int(nw == nwmax))
            if got != c.plan or (nwmax, nwgran, tpw) != K.BLOCK[(c.tdt, c.cdt, c.C)]:
                wrong.append(f"{c.id}: claims {c.plan} {K.BLOCK[(c.tdt, c.cdt, c.C)]}, planned {got} {(nwmax, nwgran, tpw)}")
            # rows on 128-byte lines get write-through stores, others plain ones
            assert mode == (2 if _pitch(w, c.cdt, aligned) * K.BYTES[c.cdt] % 128 == 0 else 0), c.id
        assert nchunks == -(-w // (nw * tpw)) and nstrip * nw >= tiles > (nstrip - 1) * nw, c.id
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("cfg", K.CONFIGS, ids=lambda c: f"{K.SHORT[c[0]]}-{K.SHORT[c[1]]}-C{c[2]}")
def test_coverage_of_a_configuration(planned, cfg):
    """on the planner's own numbers, not the claimed ones"""
    two_waves = cfg == ("float32", "float32", 384)
    mine = [c for c in K.all_cases() if (c.tdt, c.cdt, c.C) == cfg]
    for form in K.FORMS:
        plans = []
        for c in mine:
            if c.form == form:
                nstrip, nw, nchunks, _, nwmax, _, _ = planned[(c.id, True)]
                plans.append((nstrip, nw, nchunks, nstrip * nw - (c.dims[2] + 31) // 32, nwmax))
        assert any(nw == nwmax for _, nw, _, _, nwmax in plans), "no case launches the widest block"
        assert any(idle > 0 for _, _, _, idle, _ in plans), "no case has a wave past the row end"
        if not two_waves:
            assert any(nchunks > 1 and nw > 2 for _, nw, nchunks, _, _ in plans), "no case walks chunks on a block of more than two waves"
            assert all(nw > 2 for _, nw, _, _, _ in plans), "a case is back on a block of two waves or fewer"
        assert any(nstrip > 1 for nstrip, _, _, _, _ in plans)


def test_shapes_are_what_the_header_of_the_cases_says(planned):
    blocks = lambda c: c.dims[0] * c.dims[1] * c.plan.nstrip
    assert all(blocks(c) % 8 for c in K.cases(shapes="B")), "shape B: every grid has a remainder over the 8 XCDs"
    assert blocks(K.cases(shapes="B", pairs=[("float32", "float32")], Cs=[192])[0]) == 603
    assert K.SHAPES["B"][2] % 64 == 8 and K.SHAPES["D"][2] % 64 == 8        # the last pair is a single tile, 8 columns wide
    for c in K.cases(shapes="AC", Cs=[128, 256]):                          # the banded cases: pair_of runs with wv >= 2 * npair at band 0
        assert c.plan.nw >= 3, c.id
    a384 = K.cases(shapes="A", pairs=[("float16", "float16")], Cs=[384])[0]
    assert a384.plan == K.Plan(2, 6, 4, 2, 0) and K.SHAPES["A"][2] - 3 * a384.tj <= 32      # a one-tile last chunk


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def test_reference_against_numpy():
    case = K.cases(shapes="D", pairs=[("float16", "float16")], Cs=[64], forms=["ln"])[0]
    inp = K.inputs(case.shape, case.tdt, case.C, "cpu", ROWS)
    ref = K.reference(case, "cpu", ROWS)
    assert ref.cv.dtype == ref.bound.dtype == torch.float64 and ref.cv.shape == (1, 2, 72, 72)
    x = inp.tokens.numpy().astype(np.float64)
    g, b = inp.gamma.numpy().astype(np.float64), inp.beta.numpy().astype(np.float64)
    y = (x - x.mean(-1, keepdims=True)) / np.sqrt(x.var(-1, keepdims=True) + 1e-5) * g + b
    cv = np.einsum("bhic,bhjc->bhij", y[:1], y[1:])
    assert np.abs(ref.cv.numpy() - cv).max() < 1e-11
    pre = K.reference(case._replace(form="pre"), "cpu", ROWS)
    assert np.abs(pre.cv.numpy() - np.einsum("bhic,bhjc->bhij", x[:1], x[1:])).max() < 1e-10
    # the bound, term by term, at one element
    S = (np.abs(y[0, 1, 5]) * np.abs(y[1, 1, 9])).sum()
    e = np.floor(np.log2(abs(cv[0, 1, 5, 9])))
    want = 64 * 2.0 ** -24 * S + (2 * 2.0 ** -11 + 2.0 ** -22) * S + 2e-5 * (np.abs(y[0, 1, 5]).sum() + np.abs(y[1, 1, 9]).sum()) + 0.5 * 2.0 ** (e - 10)
    assert abs(float(ref.bound[0, 1, 5, 9]) - want) < 1e-12 * want
    S = (np.abs(x[0, 1, 5]) * np.abs(x[1, 1, 9])).sum()
    e = np.floor(np.log2(abs(float(pre.cv[0, 1, 5, 9]))))
    assert abs(float(pre.bound[0, 1, 5, 9]) - (64 * 2.0 ** -24 * S + 0.5 * 2.0 ** (e - 10))) < 1e-12


def test_inputs_are_what_the_cases_say():
    inp = K.inputs("A", "float16", 128, "cpu", ROWS)
    x = inp.tokens.float()
    assert inp.tokens.dtype == torch.float16 and x.shape == (2, 2, 304, 128)
    m = x.mean(-1)
    assert float(m[:, :, 5::37].min()) > 5.5 and float(m[:1, :, 6:37].abs().max()) < 1.2          # a few tokens four standard deviations up
    a, b = K.operands(inp, "ln")
    cv = K.product64(a, b)
    assert float(cv[0, 0, 10, 7]) > 100 and float(cv[0, 0].abs().median()) < 20                    # matches near C among N(0, sqrt(C))


# ---- the emulation and its wrong variants -------------------------------------------------------------------------------------------------
def _trunc16(v):
    """fp32 -> fp16 towards zero"""
    h = v.half()
    bits = h.view(torch.int16)
    return torch.where(h.float().abs() > v.abs(), bits - 1, bits).view(torch.float16)


def emulate(case, inp, mut=None):
    """K1's arithmetic in torch on the CPU; ``mut`` switches ONE deliberate mistake on (None where the case has no such path)"""
    B, tdt, C = inp.B, K.TDT[case.tdt], case.C
    w, nw, tj = case.dims[2], case.plan.nw, case.tj
    x = inp.tokens.float()
    if case.form == "ln":
        d = x - x.mean(-1, keepdim=True)
        var = (d * d).sum(-1, keepdim=True) / (C - 1 if mut == "unbiased" else C)
        n = d * torch.rsqrt(var + 1e-5)
        y = n * inp.gamma + inp.beta
        if mut == "right_affine":
            y[B:] = n[B:]
        x = y.to(tdt).float()
    elif mut in ("unbiased", "right_affine"):
        return None
    a, b = x[:B], x[B:]
    i, j = torch.arange(w), torch.arange(w)
    if mut == "chunk0":                                                # the right tokens of chunk c >= 1 taken from chunk 0
        if case.plan.nchunks < 2:
            return None
        b = b[:, :, j % tj]
    if mut == "ragged_shift":                                          # the last column tile shifted by one token
        last = (w - 1) // 32 * 32
        b = b[:, :, torch.where(j >= last, (j - 1), j)]
    if mut == "strip":                                                 # rows of strip 1 written by strip 0's waves
        if case.plan.nstrip < 2:
            return None
        a = a[:, :, torch.where((i >= 32 * nw) & (i < 64 * nw), i - 32 * nw, i)]
    cv = torch.matmul(a, b.transpose(-1, -2))
    if mut == "kstep":                                                 # a 16-channel k-step dropped in one 32-column tile
        cv[..., 32:64] -= torch.matmul(a[..., 16:32], b[:, :, 32:64, 16:32].transpose(-1, -2))
    if mut == "trunc16":
        if (case.form, case.tdt, case.cdt) != ("pre", "float16", "float16"):
            return None
        return _trunc16(cv)
    return cv.to(K.TDT[case.cdt])


def _run(case, mut=None):
    inp = K.inputs(case.shape, case.tdt, case.C, "cpu", ROWS)
    out = emulate(case, inp, mut)
    return None if out is None else K.compare(out, K.reference(case, "cpu", ROWS))


@pytest.mark.parametrize("case", K.all_cases(), ids=lambda c: c.id)
def test_emulation_passes_and_wrong_variants_fail(case):
    res = _run(case)
    print(K.line(case, res))
    assert res.ratio <= 1, K.line(case, res)
    applied = 0
    for mut in MUTATIONS:
        r = _run(case, mut)
        if r is None:
            continue
        applied += 1
        print(f"    {mut:13s} {MUTATIONS[mut]}: ratio {r.ratio:.3g}, {r.nbad} of {r.n} elements over the bound")
        assert r.ratio > 1, f"{case.id}: '{MUTATIONS[mut]}' passes"
    assert applied >= 2


MUTATIONS = {
    "kstep": "a 16-channel k-step dropped in one 32-column tile",
    "chunk0": "the right tokens of chunk c >= 1 taken from chunk 0",
    "ragged_shift": "the last column tile shifted by one token",
    "strip": "rows of one strip written by the neighbouring strip's wave (left index off by 32 * NW)",
    "trunc16": "the fp16 output truncated instead of rounded",
    "unbiased": "LayerNorm with the unbiased variance",
    "right_affine": "gamma / beta of the right image skipped",
}


def test_every_mutation_applies_somewhere():
    for mut in MUTATIONS:
        n = sum(_run(c, mut) is not None for c in K.cases(shapes="AD"))
        assert n >= 4, mut


def test_truncation_is_caught_only_without_the_layernorm_terms():
    """why the prenorm fp16 -> fp16 cases are there: the LN-form bound has room for a truncated output"""
    case = K.cases(shapes="A", pairs=[("float16", "float16")], Cs=[128], forms=["pre"])[0]
    r = _run(case, "trunc16")
    assert 0.05 < r.nbad / r.n < 0.6, r


# ---- band ---------------------------------------------------------------------------------------------------------------------------------
def test_band_masks():
    case = K.cases(shapes="A", pairs=[("float16", "float16")], Cs=[256], forms=["ln"])[0]      # 10 waves, chunks of 160 columns
    assert case.tj == 160
    inside, beyond = K.band_masks(case, 11)
    assert not bool((inside & beyond).any())
    assert bool(beyond[0, 64:160].all()) and not bool(beyond[0, :64].any())          # rows 0 .. 31 need columns 0 .. 42: one pair
    assert bool(beyond[0, 160:].all())                                               # and nothing of the second chunk
    assert not bool(beyond[160, 160:224].any()) and bool(beyond[160, 224:].all())    # rows 160 .. 191 need up to column 202: one pair of chunk 1
    assert not bool(beyond[160, :160].any())
    # rows 96 .. 127 need up to column 138: the third pair of chunk 0, columns 128 .. 191 -- 32 columns into chunk 1 (five tiles per chunk)
    assert not bool(beyond[96, :192].any()) and bool(beyond[96, 192:].all()) and not bool(inside[96, 160:].any())
    # one chunk (tj >= w): the rule of tests/test_hip_dispinit.py, (i | 31) + band + 64 rounded down to the granule
    one = K.cases(shapes="A", pairs=[("float16", "float16")], Cs=[128], forms=["ln"])[0]
    inside, beyond = K.band_masks(one, 11)
    i = torch.arange(304)[:, None]
    j = torch.arange(304)[None, :]
    assert bool(beyond[j >= (i | 31) + 11 + 64].all()) and not bool((inside & beyond).any())
    for band in (0, 75, 309):
        inside, beyond = K.band_masks(case, band)
        assert not bool((inside & beyond).any())
    assert bool(inside.all()) and not bool(beyond.any())                              # band >= w: everything
