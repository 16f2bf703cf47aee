"""Cases, plain operands, inputs, the float64 reference, a float64 emulation of the kernel's rounding points (with deliberately wrong variants),
the bounds and the one comparator of K9 (s2m2_mlp_chain, csrc/chain.hip), shared by tests/test_hip_k9_chain.py (the kernel through the raw C
entry) and tests/test_k9_cases_cpu.py (coverage of the forms as the host selector chooses them, the claims of the exact regime, the emulation
through this comparator, the leave-one-out check of the ensemble bound and the rejection of every wrong variant): what rejects a wrong
variant on the CPU is literally what the GPU test runs.  The pieces that exist are taken from tests/k5_cases.py (bound(), ulp(), GELU_ABS,
LIPSCHITZ), tests/k13_cases.py (Rounder, ln_stats, ln_fold_bound, ln_out_bound, token_bound, compare) and tests/test_select_cpu.py (the host
program that prints what csrc/chain_select.h selects).

Operands      A case is built from PLAIN tensors (operands()): (C, C) layers in the I/O dtype, fp32 biases or None, the ln_out affine.  The
              reference never sees a packed tensor.  The kernel gets pack.pack_conv / pack.chain_frag / pack.pack_bias of them and wsum, the
              row sums of the ROUNDED packed weight, exactly as engine.Layer derives them (packed(); tests/test_k9_cases_cpu.py asserts the
              equality on one layer of seeded_state_dict).
Inputs        x and res are channel slices of rows 1 .. n of wider buffers whose every other element is GUARD (200): a read outside the rows
              changes a result and stays inside the allocation.  Pooled cases: x is images 1 .. N of an (N + 2, H, W, x_stride) buffer.
Reference     reference(): float64 on the rounded inputs, true two-pass LayerNorm, no intermediate rounding:
              y_s = act_s(W_s (LN?)(t_s) + b_s), + res at res_stage, + y_0 on stage 2 with carry, out, ln_out = LN(out) g + b,
              fan_f = W_f (LN?)(out) + b_f; with pooling x is the exact mean of the four pixels of the floor grid.
Emulation     emulate(): float64 arithmetic that rounds to the I/O dtype at exactly the points R1 .. R6 the header of chain.hip lists, with the
              fold rstd (acc - mean wsum) + b and the statistics taken as the kernel takes them (fold_stats(): fp16 -- one-pass fp32 sums per
              half-wave in the order of the k16 steps, the halves added, q / C - mean^2 clamped at 0; fp32 -- the same sums about the row's
              first element); the fan-out layers use the statistics of the stored rows; ln_out is two-pass on the stored rows.  flips=seed
              moves rounded non-zero intermediates to a neighbouring value with probability 1/8 each way, except the sums of two I/O-dtype
              values (k13_cases argues why).

Regimes
  exact       no LayerNorm, NONE / RELU.  Integer activations (+-1, +-2), an integer residual (+-1, +-2), weights in {-1, 0, 1} thinned to
              EXACT_NNZ[depth] non-zeros per output channel at seeded positions (depth = layers in front; 16, 6, 4, 2: the worst case
              2 * 16 + 4 + 2 = 38, 6 * 38 + 4 + 2 = 234, 4 * 234 + 4 + 2 + 38 = 984, 2 * 984 + 4 = 1972), integer biases |b| <= 4.  operands()
              asserts sum |w| |t| + |b| (+ |res|, + |y_0|) <= 2048 at every stage and fan-out layer on the case's own rows, reference()
              asserts ref.to(dtype) == ref.  The kernel owes every bit and +0.0 for zero.  With pooling the four pixels of a pooled integer
              p are p + a, p - a, p + b, p - b (integers; their sum is 4 p, asserted): the mean is the integer p without rounding.  The
              non-zeros of an output channel sit at seeded positions of their own, so neighbouring couts and neighbouring k16 steps differ;
              that one swapped k16 half, cout tile, stage weight or fan-out layer changes an integer is shown by the wrong variants.
              (The chain `attn_tail` has a LayerNorm and a GELU; its exact form keeps the three stages, res_stage 0 and the carry, with RELU
              in place of GELU and no LayerNorm.)
  gauss       layers N(0, 1 / C), biases N(0, 0.3^2), ln_out affine (1 + 0.1 N, 0.05 N), res N(0, 1).  Row r has offset
              OFFS[(r + 2 (r // 32)) % 3] and scale SCALES[r % 2]: neighbours inside one 32-row MFMA tile differ in both.  Row CONST_ROW
              (or the last; none in a one-row case) is the constant 1.5: variance exactly 0, rstd = eps^-1/2.  Row QUIET_ROW is N(0, 2^-16): its variance is of the
              size of eps, so a wrong eps shows.  In `hot` cases (fp16) row HOT_ROW is the constant HOT[C], an 11-bit value whose one-pass
              fp32 variance is NEGATIVE in the order fold_stats() sums it (found by hot_search(), asserted on the CPU for every width: one
              exists for each of 128 / 192 / 256 / 384 / 512).
              Measured on the S model's forward (CPU oracle, synthetic_pair(128, 192), seeded weights, all levels): see CHAIN_RATIO.
  pass        one stage with the identity weight, no bias, NONE, ln_out on: out must equal x bit for bit, ln_out is judged by ln_out_bound();
              rows 64 + k / 16: |mean| / std of 500.

Bounds        Every element is judged, non-finite fails, nothing is measured on the kernel.
  exact       equality of bits; the ln_out of such rows is judged by ln_out_bound() with E = 0.
  analytic    one-stage cases, fan-out-only cases, the pass probe and every fp32 case: stage_bound() per layer --
                accumulation, activation, staging   k5_cases.bound() (K = C);
                a folded LayerNorm                  k13_cases.ln_fold_bound() in place of the accumulation term, + u |b| for the bias fma.
                                                    fp32 rows: the kernel takes its sums about the row's first element x0, so the bound is
                                                    evaluated on x - x0 (M2 is then the second moment about x0) and the product terms, which
                                                    the kernel forms on the raw row, are added: 2 rstd [(C + 2) u |W||x| + 4 u (|acc| + |m ws|)].
                                                    A constant row (v = 0) makes r hit its clamp; the bound still holds there: the kernel's
                                                    variance lies in [0, dvar], so its rstd is at most eps^-1/2 = the true one, and
                                                    |y - b| = rstd |acc - mean ws| is at most the product terms, which the formula keeps.
                an input that carries an error e    |W| e without LayerNorm; with it |W| dn, dn = 1.02 (e + mean e + |n| rms e) / sigma (the
                                                    first-order term of ln_out_bound()).  Pooling: e = half an ulp of the I/O dtype at the mean
                                                    + 3 u mean|pixels| (the three fp32 additions).
                a sum with res / y_0                K5's ADD term u |o| + half an ulp of the result, plus the error of the operand added.
                GELU in fp32 outside [-8, 8]        epilogue.h states 0.75e-7 |x| for fast_gelu; that is added to GELU_ABS.
              fp32 chains of 2 - 3 stages propagate this stage by stage; it is loose by construction and the table shows by how much.
              ln_out: k13_cases.ln_out_bound() of the bound of `out`, plus the error of the fp32 mean (ln_out_bound9()).  FINDING: a correct
              kernel exceeded ln_out_bound() alone on the pass probe at C = 192 (err 4.8e-5 against 1.4e-5).  Its term (C + 8) u (|n| + 1) is
              relative to the centred row, but the mean's own error is relative to |mean|: depth u mean|x| from the summation tree and
              2 u |mean| from sum * fl(1 / 192), which is not exact as sum / 128 is; over sigma that is |mean| / std = 500 times larger.  At
              C = 128 / 256 / 512 the probe's rows (multiples of 1/16 near 64) sum exactly in fp32, which is why K13's probe never met it.
  ensemble    fp16 chains of 2 - 3 stages and fan-out layers behind a chain: per row ulp16(max(1, |R|)) + 2 D_row (k13_cases.token_bound()),
              D_row the largest |E - R| over the row's channels across the round-to-nearest emulation and eight flipped ones.  The CPU test
              shows the factor 2 neither too tight (leave-one-out) nor too loose (every wrong variant fails).

Forms         chosen(case) is what csrc/chain_select.h selects on the host (the program of tests/test_select_cpu.py); every case names the form
              and tile height it is meant for and the tests assert the selection.  Staged fp16 (C, BM): (128, 32) (128, 64) (256, 32)
              (256, 64) (384, 32) (512, 32); staged fp32 (128, 32) (256, 32); direct and fan-only (128, 32) (128, 64) (192, 32) (192, 64)
              (256, 32) (256, 64) (384, 32) (512, 32).  Tall tiles are reached by the row count alone: T + 1 and T + 64 + 37 rows (the last
              tile holds 1, respectively 37 rows) and exactly T rows, which must select the 32-row tile.  The direct form at C = 384 with
              64-row tiles is compiled but no row count selects it: it is not tested.
Wrong kernels VARIANTS, each expressed in emulate(); applies() says which cases have the feature a variant breaks, exempt() which of those
              cannot show it.  NOT_SHOWN lists what the issue names but no float64 comparison can show, and why.
"""
import collections
import functools
import math
import zlib

import numpy as np
import torch

import k5_cases as K5
import k13_cases as K13
from s2m2_amd import pack

EPS = 1e-5
LN_OUT_EPS = 1e-5
GUARD = 200.0
OFFS = (0.0, 1.0, 4.0)
SCALES = (0.25, 1.5)
# largest |mean| / std of a row that enters a folded LayerNorm or the ln_out of a K9 launch in the S forward -- every pre-LayerNorm of the
# transformer (z' in front of each FFN, the rows in front of each Q | K | V) and feature_tr_4x in front of DispInit's LayerNorm; CPU oracle
# (oracle.s2m2_oracle.forward with _ln and ln_corr wrapped to record their input; tests/test_k9_cases_cpu.py repeats the measurement),
# synthetic_pair(128, 192), seeded weights.  Per level: 1/4 (128 channels, 3072 tokens) 0.32; 1/8 (128 channels, 768 tokens) 0.18; the 2-D
# blocks at 1/16 and 1/32 (256 channels, 192 / 48 / 24 tokens) 0.15 / 0.15 / 0.13, 128 channels on 24 tokens 0.22; feature_tr_4x 0.18.
# The stress range max(OFFS) / min(SCALES) = 16 is far above twice that.
CHAIN_RATIO = 0.33
CONST_ROW, QUIET_ROW, HOT_ROW = 5, 2, 7
HOT = {128: 8.0078125, 192: 8.0078125, 256: 8.0078125, 384: 8.0078125, 512: 8.0078125}   # checked by hot_search() in the CPU test
FLIP_SEEDS = tuple(range(1, 9))
EXACT_NNZ = (16, 6, 4, 2)
TDT = K5.TDT
F16, F32 = "float16", "float32"
DT_CODE = {F32: 0, F16: 1}                                     # S2M2_F32 / S2M2_F16
NONE, GELU, RELU = K5.ACT_NONE, K5.ACT_GELU, K5.ACT_RELU
TALL_T = {("staged", 128): 8192, ("staged", 256): 8192, ("direct", 128): 24576, ("direct", 192): 16384, ("direct", 256): 8192}

Chain = collections.namedtuple("Chain", "acts ln bias res_stage carry")
CHAINS = {
    "attn_tail": Chain((NONE, GELU, NONE), (0, 1, 0), (1, 1, 1), 0, 1),
    "conv1x1": Chain((RELU, NONE), (0, 0), (1, 1), -1, 0),
    "ctx": Chain((GELU, NONE), (0, 0), (1, 1), -1, 0),
    "norm_only": Chain((NONE,), (0,), (1,), -1, 0),
    "res1": Chain((NONE,), (0,), (1,), 0, 0),
    "plain1": Chain((NONE,), (0,), (1,), -1, 0),
    "pooled": Chain((NONE,), (0,), (1,), -1, 0),
    "fan": Chain((), (), (), -1, 0),
    "pass": Chain((NONE,), (0,), (0,), -1, 0),
    # what the descriptor promises and the engine does not use
    "res_last2": Chain((RELU, NONE), (0, 0), (1, 1), 1, 0),
    "res_last3": Chain((NONE, RELU, NONE), (0, 0, 0), (1, 1, 1), 2, 0),
    "res_last3c": Chain((NONE, RELU, NONE), (0, 0, 0), (1, 1, 1), 2, 1),
    "ln0": Chain((NONE, RELU), (1, 0), (1, 1), -1, 0),                  # LN on stage 0, RELU on the last stage
    "ln2": Chain((RELU, NONE, NONE), (0, 0, 1), (1, 0, 1), 0, 1),       # LN on stage 2, a stage without bias
}


class Case(collections.namedtuple("Case", "C dtype frag bm rows chain regime nfan fan_ln fan_bias ln_out xcd pool xs rs os ls fs hot")):
    @property
    def form(self):
        return "fan_only" if self.nstage == 0 else "direct" if self.frag else "staged"

    @property
    def id(self):
        s = f"{self.form}-C{self.C}-{K5.SHORT[self.dtype]}-bm{self.bm}-r{self.rows}-{self.chain}-{self.regime}"
        if self.nfan:
            s += f"-fan{self.nfan}" + ("ln" if self.fan_ln else "") + ("" if self.fan_bias else "nb")
        s += ("-lnout" if self.ln_out else "") + (f"-xcd{self.xcd}" if self.xcd else "") + ("-pool%dx%dx%d" % self.pool if self.pool else "")
        s += f"-xs{self.xs}" + (f"-rs{self.rs}" if self.ch.res_stage >= 0 else "") + (f"-os{self.os}" if self.nstage else "")
        s += (f"-ls{self.ls}" if self.ln_out else "") + (f"-fs{self.fs}" if self.nfan else "") + ("-hot" if self.hot else "")
        return s

    @property
    def ch(self):
        c = CHAINS[self.chain]
        if self.regime == "exact":                                                   # no LayerNorm, no GELU
            c = c._replace(acts=tuple(RELU if a == GELU else a for a in c.acts), ln=tuple(0 for _ in c.ln))
        return c

    @property
    def nstage(self):
        return len(CHAINS[self.chain].acts)

    @property
    def any_ln(self):
        return bool(any(self.ch.ln) or (self.nfan and self.fan_ln))

    @property
    def ln_rows(self):
        """how the constant, quiet and hot rows reach a folded LayerNorm: 'x' -- it reads the x rows (LN on stage 0, fan-out only); 'res' -- it
        reads y_0 = b_0 + res of rows whose x is 0 (LN on stage 1 behind res_stage 0: attn_tail); None -- they do not reach one"""
        ch = self.ch
        if (self.nstage == 0 and self.nfan and self.fan_ln) or (self.nstage and ch.ln[0]):
            return "x"
        if self.nstage >= 2 and ch.ln[1] and ch.res_stage == 0 and ch.acts[0] == NONE and ch.bias[0]:
            return "res"
        return None

    @property
    def kind(self):
        """which bound judges the case"""
        if self.regime == "exact":
            return "exact"
        deep = self.nstage + (1 if self.nfan else 0)
        return "ensemble" if (self.dtype == F16 and deep >= 2) else "analytic"

    @property
    def descriptor(self):
        """the launch as the host program of tests/test_select_cpu.py reads it"""
        return (f"chain C={self.C} dtype={DT_CODE[self.dtype]} rows={self.rows} nstage={self.nstage} nfan={self.nfan} weight_frag={int(self.frag)} "
                f"xcd_group_rows={self.xcd}")

    @property
    def expected(self):
        nw = self.C // 32 if self.frag else (4 if self.C in (128, 384) else 8)
        xt = self.xcd // self.bm if (self.xcd and self.form != "fan_only" and self.xcd % self.bm == 0 and self.rows % (8 * self.xcd) == 0) else 0
        return f"{self.form} BM={self.bm} NW={nw} WP={0 if self.frag else 4} xcd={xt}"

    @property
    def xcd_tiles(self):
        return int(self.expected.rsplit("=", 1)[1])


def pad_of(stride, width):
    """channels of guard in front of a slice of `width` channels inside rows of `stride` (16-byte aligned in both dtypes)"""
    return (stride - width) // 16 * 8


def _mk(C, dtype, frag, bm, rows, chain, regime, nfan=0, fan_ln=False, fan_bias=True, ln_out=False, xcd=0, pool=None, k=0, hot=None):
    """strides rotate with k so that every non-minimal one appears in every family"""
    xs = (C, C + 8, 3 * C)[k % 3]
    rs = (C + 16, C)[(k // 3) % 2]
    os_ = (C + 8, C)[(k // 2) % 2]
    ls = (C + 24, C)[(k // 5) % 2]
    fs = nfan * C + (8, 0)[(k // 2 + k // 3) % 2] if nfan else 0
    c = Case(C, dtype, frag, bm, rows, chain, regime, nfan, fan_ln, fan_bias, ln_out, xcd, pool, xs, rs, os_, ls, fs, False)
    if hot is None:
        hot = regime == "gauss" and dtype == F16 and c.ln_rows is not None and rows > HOT_ROW
    return c._replace(hot=bool(hot))


STAGED16 = ((128, 32), (128, 64), (256, 32), (256, 64), (384, 32), (512, 32))
STAGED32 = ((128, 32), (256, 32))
DIRECT = ((128, 32), (128, 64), (192, 32), (192, 64), (256, 32), (256, 64), (384, 32), (512, 32))
SHORT_ROWS = (1, 31, 32, 33, 97)
POOL_GRIDS = ((1, 2, 2), (1, 3, 5), (2, 8, 18), (1, 9, 15))


def row_counts(form, C, bm):
    if bm == 32:
        return (33, 97)
    T = TALL_T[("direct" if form == "fan_only" else form, C)]
    return (T + 1, T + 64 + 37)


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    k = 0

    def add(*a, **kw):
        nonlocal k
        out.append(_mk(*a, k=k, **kw))
        k += 1

    families = [("staged", F16, False, f) for f in STAGED16] + [("staged", F32, False, f) for f in STAGED32] + [("direct", F16, True, f) for f in DIRECT]
    # attn_tail on every form: two row counts, exact and gauss, with the fan-out of the next block / its own bias / nothing
    for form, dt, frag, (C, bm) in families:
        for i, rows in enumerate(row_counts(form, C, bm)):
            for regime in ("exact", "gauss"):
                fan = dict(nfan=3, fan_ln=regime == "gauss") if i == 0 else dict(nfan=1, fan_ln=False, fan_bias=True)
                add(C, dt, frag, bm, rows, "attn_tail", regime, **fan)
        if bm == 64:                                                                 # exactly T rows: the 32-row tile
            add(C, dt, frag, 32, TALL_T[(form, C)], "plain1", "exact")
    # attn_tail with ln_out and the XCD hint: rows = 2 images x 8 groups x g rows
    for (form, dt, frag, C), g in ((("staged", F16, False, 128), 64), (("direct", F16, True, 256), 64), (("direct", F16, True, 192), 32),
                                   (("direct", F16, True, 192), 64), (("staged", F32, False, 128), 64), (("staged", F16, False, 384), 32),
                                   (("direct", F16, True, 512), 64), (("direct", F16, True, 128), 48)):     # 48: no tile multiple, ignored
        add(C, dt, frag, 32, 16 * g, "attn_tail", "gauss", ln_out=True, xcd=g)
    add(128, F16, True, 32, 16 * 64, "attn_tail", "exact", ln_out=False, xcd=64)
    # every other chain on staged fp16 C = 128, direct C = 256, direct C = 192 and one fp32 form
    four = (("staged", F16, False, 128), ("direct", F16, True, 256), ("direct", F16, True, 192), ("staged", F32, False, 128))
    j = 0
    for chain in ("conv1x1", "ctx", "norm_only", "res1", "plain1", "res_last2", "res_last3", "res_last3c", "ln0", "ln2"):
        for form, dt, frag, C in four:
            rows = SHORT_ROWS[j % 5]
            j += 1
            opts = {}
            if chain == "norm_only":
                opts = dict(ln_out=True, xcd=32 if j % 2 else 0)
                rows = 512 if opts["xcd"] else rows
            if chain in ("ln0", "ln2") and j % 2:
                opts = dict(nfan=(2, 4)[j % 4 // 2], fan_ln=True)
            if chain in ("res_last2", "res_last3c") and j % 2 == 0:
                opts = dict(nfan=(4, 2)[j % 4 // 2], fan_ln=False, fan_bias=False)
            if CHAINS[chain].acts.count(GELU) == 0 and not any(CHAINS[chain].ln) and not opts.get("fan_ln"):
                add(C, dt, frag, 32, rows, chain, "exact", **opts)
            add(C, dt, frag, 32, rows, chain, "gauss", **opts)
    # norm_only at the widths whose ln_out takes the second pass (24 / 48 pieces) and the widest
    for C, frag in ((384, True), (384, False), (512, True), (256, False)):
        add(C, F16, frag, 32, SHORT_ROWS[k % 5], "norm_only", "gauss", ln_out=True)
    add(256, F32, False, 32, 33, "norm_only", "gauss", ln_out=True)
    add(256, F32, False, 32, 97, "ctx", "gauss")
    add(256, F32, False, 32, 33, "ln0", "gauss", nfan=2, fan_ln=True)
    # one-stage chains at every short row count on one staged and one direct form
    for rows in SHORT_ROWS:
        add(128, F16, False, 32, rows, "res1", "gauss")
        add(256, F16, True, 32, rows, "plain1", "exact")
    # fan-out only: nfan 1 - 4, with and without LN, every form
    for n, (C, bm) in enumerate(DIRECT):
        counts = row_counts("fan_only", C, bm) if bm == 64 else (SHORT_ROWS[n % 5], SHORT_ROWS[(n + 3) % 5])
        for i, rows in enumerate(counts):
            nfan = 1 + (n + 2 * i) % 4
            add(C, F16, True, bm, rows, "fan", "gauss", nfan=nfan, fan_ln=True, fan_bias=i == 0)
            add(C, F16, True, bm, rows, "fan", "exact", nfan=1 + (nfan + 1) % 4, fan_ln=False, fan_bias=i == 1)
            add(C, F16, True, bm, rows, "fan", "gauss", nfan=1 + (nfan + 2) % 4, fan_ln=False)
        if bm == 64:
            add(C, F16, True, 32, TALL_T[("direct", C)], "fan", "exact", nfan=1, fan_ln=False)
    # pooling: the chain `pooled` (one stage, fan-out 3 with LN) and fan-out only, on the four grids
    for n, grid in enumerate(POOL_GRIDS):
        rows = grid[0] * (grid[1] // 2) * (grid[2] // 2)
        C = (128, 256, 192, 128)[n]
        add(C, F16, True, 32, rows, "pooled", "gauss", nfan=3, fan_ln=True, pool=grid)
        add(C, F16, True, 32, rows, "pooled", "exact", nfan=3, fan_ln=False, pool=grid)
        add((256, 128, 384, 512)[n], F16, True, 32, rows, "fan", "gauss", nfan=1 + n % 2, fan_ln=n % 2 == 0, pool=grid)
        add((192, 256, 128, 192)[n], F16, True, 32, rows, "fan", "exact", nfan=2 - n % 2, fan_ln=False, pool=grid)
    # the pass probe
    for C, dt, frag in ((128, F16, False), (192, F16, True), (512, F16, True), (128, F32, False), (256, F32, False)):
        add(C, dt, frag, 32, 97, "pass", "pass", ln_out=True)
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def selection():
    """descriptor -> what csrc/chain_select.h chooses for it: one run of tests/test_select_cpu.py's host program over every case"""
    import subprocess
    import tempfile

    import test_select_cpu as S
    wanted = list(dict.fromkeys(c.descriptor for c in all_cases()))
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = f"{tmp}/select.cpp", f"{tmp}/select"
        with open(src, "w") as f:
            f.write(S.PROGRAM)
        subprocess.run([S._compiler(), "-std=c++17", "-O1", "-I", S.ROOT, src, "-o", exe], check=True, capture_output=True, text=True)
        out = subprocess.run([exe], input="\n".join(wanted) + "\n", check=True, capture_output=True, text=True).stdout
    got = dict(ln.split(" -> ", 1) for ln in out.strip().splitlines())
    assert set(got) == set(wanted)
    return got


def chosen(case):
    return selection()[case.descriptor]


# ---- plain operands ------------------------------------------------------------------------------------------------------------------------
Ops = collections.namedtuple("Ops", "W b fanW fanb gout bout")      # W: nstage (C, C) in the I/O dtype; b: fp32 or None; fanW (nfan, C, C); fanb (nfan*C) or None


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _sparse(C, nnz, g):
    """(C, C) weights in {-1, 0, 1} with nnz non-zeros per row at seeded positions of the row's own"""
    keep = torch.rand(C, C, generator=g).argsort(1).argsort(1) < nnz
    return (2.0 * torch.randint(0, 2, (C, C), generator=g) - 1.0) * keep


@functools.lru_cache(maxsize=None)
def _operands(C, dtype, chain, regime, nfan, fan_bias):
    g = torch.Generator().manual_seed(_seed("ops", C, dtype, chain, regime, nfan, fan_bias))
    rn = lambda *s: torch.randn(*s, generator=g)                                    # noqa: E731
    rnd = lambda t: t.to(TDT[dtype])                                                # noqa: E731
    ch = CHAINS[chain]
    nst = len(ch.acts)
    gout, bout = 1.0 + 0.1 * rn(C), 0.05 * rn(C)
    if regime == "pass":
        return Ops((rnd(torch.eye(C)),), (None,), None, None, gout, bout)
    if regime == "exact":
        W = tuple(rnd(_sparse(C, EXACT_NNZ[s], g)) for s in range(nst))
        b = tuple(torch.randint(-4, 5, (C,), generator=g).float() if ch.bias[s] else None for s in range(nst))
        fanW = rnd(torch.stack([_sparse(C, EXACT_NNZ[nst], g) for _ in range(nfan)])) if nfan else None
        fanb = torch.randint(-4, 5, (nfan * C,), generator=g).float() if (nfan and fan_bias) else None
    else:
        W = tuple(rnd(rn(C, C) / math.sqrt(C)) for _ in range(nst))
        b = tuple((0.3 * rn(C) * 128).round() / 128 if ch.bias[s] else None for s in range(nst))     # multiples of 2^-7: exact in either dtype
        fanW = rnd(torch.stack([rn(C, C) / math.sqrt(C) for _ in range(nfan)])) if nfan else None
        fanb = 0.3 * rn(nfan * C) if (nfan and fan_bias) else None
    return Ops(W, b, fanW, fanb, gout, bout)


def operands(case):
    return _operands(case.C, case.dtype, case.chain, case.regime, case.nfan, case.fan_bias)


Packed = collections.namedtuple("Packed", "W b wsum fanW fanb fanwsum gout bout")


def pack_layer(w, dtype, frag):
    """one plain (C, C) layer -> (what the descriptor's weight points to, the row sums of the rounded packed weight)"""
    wp = pack.pack_conv(w.float(), TDT[dtype])
    wsum = wp.float().sum(dim=1).contiguous()
    return (pack.chain_frag(wp) if frag else wp), wsum


def packed(case, device="cpu"):
    """what the entry takes, on `device` (the fragment order is formed on the CPU: the torch formula of pack.chain_frag)"""
    ops, C = operands(case), case.C
    to = lambda t: None if t is None else t.to(device).contiguous()                 # noqa: E731
    W, ws = zip(*[pack_layer(w, case.dtype, case.frag) for w in ops.W]) if ops.W else ((), ())
    b = [pack.pack_bias(bb, C) for bb in ops.b]
    fanW = fanws = None
    if case.nfan:
        pl = [pack_layer(w, case.dtype, case.frag) for w in ops.fanW]
        fanW, fanws = torch.cat([p[0] for p in pl], 0), torch.cat([p[1] for p in pl], 0)
    return Packed([to(w) for w in W], [to(t) for t in b], [to(t) for t in ws], to(fanW), to(pack.pack_bias(ops.fanb, case.nfan * C) if ops.fanb is not None else None),
                  to(fanws), to(ops.gout.float()), to(ops.bout.float()))


def wsum_of(w):
    """row sums of a plain layer as the kernel gets them: fp32 sums of the rounded values"""
    return w.float().sum(dim=1).double()


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
Inputs = collections.namedtuple("Inputs", "xbuf x rbuf res")       # x: the (rows, C) or (N, H, W, C) view the kernel reads; res: (rows, C) view or None


def _rows_plain(case, g):
    rows, C = case.rows, case.C
    if case.regime == "exact":
        return (torch.randint(1, 3, (rows, C), generator=g) * (2 * torch.randint(0, 2, (rows, C), generator=g) - 1)).float()
    if case.regime == "pass":
        return 64.0 + 0.0625 * torch.randint(0, 7, (rows, C), generator=g).float()
    r = torch.arange(rows)
    off = torch.tensor(OFFS)[(r + 2 * (r // 32)) % 3][:, None]
    sc = torch.tensor(SCALES)[r % 2][:, None]
    x = off + sc * torch.randn(rows, C, generator=g)
    if rows > QUIET_ROW:
        x[QUIET_ROW] = 2.0 ** -8 * torch.randn(C, generator=g)
    if rows > 1:
        x[min(CONST_ROW, rows - 1)] = 1.5
    if case.hot:
        x[HOT_ROW] = HOT[C]
    return x


def _fill(case):
    g = torch.Generator().manual_seed(_seed("x", case.id))
    rows, C = case.rows, case.C
    rnd = lambda t: t.to(TDT[case.dtype]).float()                                   # noqa: E731
    if case.pool is None:
        x = rnd(_rows_plain(case, g))
    else:
        N, H, W = case.pool
        Ho, Wo = H // 2, W // 2
        p = _rows_plain(case, g).reshape(N, Ho, Wo, C)
        if case.regime == "exact":
            a, b = (torch.randint(0, 3, (N, Ho, Wo, C), generator=g).float() for _ in range(2))
            quad = [p + a, p - a, p + b, p - b]
        else:
            d = [0.5 * torch.randn(N, Ho, Wo, C, generator=g) for _ in range(3)]
            quad = [p + d[0], p + d[1], p + d[2], p - d[0] - d[1] - d[2]]
        x = GUARD * torch.ones(N, H, W, C)                                           # the dropped last row / column of an odd size stay GUARD
        for i, q in enumerate(quad):
            x[:, i // 2:2 * Ho:2, i % 2:2 * Wo:2] = q
        x = rnd(x)
    res = None
    if case.ch.res_stage >= 0:
        if case.regime == "exact":
            res = (torch.randint(1, 3, (rows, C), generator=g) * (2 * torch.randint(0, 2, (rows, C), generator=g) - 1)).float()
        else:
            res = rnd(torch.randn(rows, C, generator=g))
        if case.regime == "gauss" and case.ln_rows == "res":
            # the special rows enter the LayerNorm of stage 1 as y_0 = T(T(0 + b_0) + res): b_0 is a multiple of 2^-7 below 2, so the tile is b_0
            # exactly, res = target - b_0 is a multiple of 2^-7 between 4 and 12 (the constants: exact) and the sum is the target, bit for bit
            b0 = operands(case).b[0]
            special = _rows_plain(case, torch.Generator().manual_seed(_seed("special", case.id)))
            for r in (QUIET_ROW, min(CONST_ROW, rows - 1)) + ((HOT_ROW,) if case.hot else ()):
                if 0 < rows > r:
                    x[r] = 0.0
                    res[r] = rnd(special[r] - b0)
    return x, res


def _guarded(t, stride, dtype, device):
    """t (n, C) or (N, H, W, C) -> (buffer with one guard row / image before and after and guard channels around, the view of t inside)"""
    C = t.shape[-1]
    pad = pad_of(stride, C)
    lead = t.shape[0]
    buf = torch.full((lead + 2,) + tuple(t.shape[1:-1]) + (stride,), GUARD, dtype=TDT[dtype])
    buf[1:-1, ..., pad:pad + C] = t.to(TDT[dtype])
    buf = buf.to(device)
    return buf, buf[1:-1, ..., pad:pad + C]


@functools.lru_cache(maxsize=4)
def inputs(case, device="cpu"):
    """built once and shared; nothing may write into them"""
    x, res = _fill(case)
    xbuf, xv = _guarded(x, case.xs, case.dtype, device)
    rbuf = rv = None
    if res is not None:
        rbuf, rv = _guarded(res, case.rs, case.dtype, device)
    return Inputs(xbuf, xv, rbuf, rv)


def _f32(t):
    return t.float().double()


def pooled_rows(case, inp, variant=None):
    """-> (the four pixels of every pooled row, float64 (4, rows, C)) by an explicit gather as the kernel addresses them: image base + (2 yo)
    row stride + (2 xo) pixel stride, row m = (n, yo, xo) of the (pool_h / 2, pool_w / 2) grid"""
    N, H, W = case.pool
    dev = inp.xbuf.device
    Ho, Wo = (-(-H // 2), -(-W // 2)) if variant == "pool_ceil_grid" else (H // 2, W // 2)
    m = torch.arange(case.rows, device=dev)
    n, yo, xo = m // (Ho * Wo), (m // Wo) % Ho, m % Wo
    dx = case.xs
    dy = (W // 2 if variant == "pool_row_stride_of_pooled_grid" else W) * dx
    base = H * W * case.xs + pad_of(case.xs, case.C)                                 # image 1 of the buffer, the slice's first channel
    o = base + n * (H * W * dx) + 2 * yo * dy + 2 * xo * dx
    flat = inp.xbuf.flatten()
    ch = torch.arange(case.C, device=dev)[None, :]
    return torch.stack([flat[(o + d)[:, None] + ch].double() for d in (0, dx, dy, dy + dx)])


# ---- float64 reference ---------------------------------------------------------------------------------------------------------------------
def _ln64(t, eps):
    m = t.mean(-1, keepdim=True)
    return (t - m) / torch.sqrt(t.var(-1, unbiased=False, keepdim=True) + eps)


def _act64(t, act):
    return K13._gelu64(t) if act == GELU else t.clamp(min=0) if act == RELU else t


Ref = collections.namedtuple("Ref", "out ln fan ts ys x")          # ts: the input of every stage; ys: the output of every stage (sums included); x: the rows


def _dev_ops(case, device):
    ops = operands(case)
    d = lambda t: None if t is None else t.to(device).double()                      # noqa: E731
    return Ops([d(w) for w in ops.W], [d(b) for b in ops.b], d(ops.fanW), d(ops.fanb), d(ops.gout), d(ops.bout))


@functools.lru_cache(maxsize=4)
def reference(case, device="cpu"):
    inp, ops, ch = inputs(case, device), _dev_ops(case, device), case.ch
    C = case.C
    x = pooled_rows(case, inp).mean(0) if case.pool else inp.x.double().reshape(case.rows, C)
    res = inp.res.double() if inp.res is not None else None
    t, ts, ys = x, [], []
    for s in range(case.nstage):
        ts.append(t)
        y = (_ln64(t, EPS) if ch.ln[s] else t) @ ops.W[s].T
        y = _act64(y + ops.b[s] if ops.b[s] is not None else y, ch.acts[s])
        if s == ch.res_stage:
            y = y + res
        if ch.carry and s == 2:
            y = y + ys[0]
        ys.append(y)
        t = y
    out = t + 0.0 if case.nstage else None
    ln = fan = None
    if case.ln_out:
        ln = _ln64(out, LN_OUT_EPS) * ops.gout + ops.bout
    if case.nfan:
        a = _ln64(t, EPS) if case.fan_ln else t
        fan = torch.cat([a @ ops.fanW[f].T for f in range(case.nfan)], -1)
        fan = (fan + ops.fanb if ops.fanb is not None else fan) + 0.0
    if case.regime == "exact":
        for o in (out, fan):
            assert o is None or torch.equal(o.to(TDT[case.dtype]).double(), o), case.id      # representable: the kernel owes every bit
    return Ref(out, ln, fan, ts, ys, x)


def exact_sums(case, device="cpu"):
    """the largest sum |w| |t| + |b| (+ |res|, + |y_0|) over the stages and fan-out layers of an exact case, and whether every pooled sum is 4 p"""
    assert case.regime == "exact"
    inp, ops, ch, ref = inputs(case, device), _dev_ops(case, device), case.ch, reference(case, device)
    top = 0.0
    for s in range(case.nstage):
        S = ref.ts[s].abs() @ ops.W[s].abs().T + (ops.b[s].abs() if ops.b[s] is not None else 0.0)
        if s == ch.res_stage:
            S = S + inp.res.double().abs()
        if ch.carry and s == 2:
            S = S + ref.ys[0].abs()
        top = max(top, float(S.max()))
    if case.nfan:
        t = ref.out if case.nstage else ref.x
        for f in range(case.nfan):
            S = t.abs() @ ops.fanW[f].abs().T + (ops.fanb[f * case.C:(f + 1) * case.C].abs() if ops.fanb is not None else 0.0)
            top = max(top, float(S.max()))
    pooled_ok = True
    if case.pool:
        q = pooled_rows(case, inp)
        pooled_ok = bool((q == q.round()).all()) and bool((q.sum(0) == 4 * ref.x).all()) and bool((ref.x == ref.x.round()).all())
    return top, pooled_ok


# ---- emulation of the kernel's arithmetic, and wrong variants of it ----------------------------------------------------------------------
VARIANTS = ("k16_halves_swapped", "frag_tile_stride", "stage_weights_shifted", "fan_weight_of_layer0", "fan_bias_of_layer0", "fan_wsum_of_layer0",
            "fan_stats_from_input", "fan_reads_unrounded", "carry_before_residual", "res_on_wrong_stage", "ln_no_clamp", "ln_eps_1e-6",
            "ln_unbiased_variance", "ln_out_stats_of_neighbour_row", "pool_ceil_grid", "pool_sum_not_mean", "pool_row_stride_of_pooled_grid",
            "tile_rows_from_next_image")
# named by the issue, absent from VARIANTS:
NOT_SHOWN = {
    "ln_out_from_unrounded": "ln_out taken from the fp32 sum before it is rounded to the I/O dtype is CLOSER to LayerNorm(out) of the float64 reference than the "
                             "kernel's own LayerNorm of the stored rows; ln_out_bound() has to admit the rounding of the rows (E / sigma), so no float64 "
                             "comparison can reject it, and where out is exact (the pass probe, E = 0) the two coincide.  tests/test_k9_cases_cpu.py shows "
                             "that emulate(variant='ln_out_from_unrounded') passes.",
    "last_tile_stores_all_rows": "rejected by the guards around the outputs, not by the comparator: tests/test_hip_k9_chain.py owns it "
                                 "(outside_is_nan()), tests/test_k9_cases_cpu.py checks the guard logic on a fake output.",
}


def tile_of_block(case, b):
    """the row tile block b works on (chain.hip: the XCD placement)"""
    xt = case.xcd_tiles
    if not xt:
        return b
    x, k = b & 7, b >> 3
    img, r = k // xt, k % xt
    return (img * 8 + x) * xt + r


def applies(variant, case):
    """does the case have the feature the variant breaks?"""
    ch, nst = case.ch, case.nstage
    last = nst - 1
    return {
        "k16_halves_swapped": case.regime != "pass", "frag_tile_stride": True, "stage_weights_shifted": nst >= 2,
        "fan_weight_of_layer0": case.nfan >= 2, "fan_bias_of_layer0": case.nfan >= 2 and case.fan_bias, "fan_wsum_of_layer0": case.nfan >= 2 and case.fan_ln,
        "fan_stats_from_input": bool(case.nfan and case.fan_ln and nst >= 1),
        "fan_reads_unrounded": bool(case.nfan and nst >= 1 and (ch.carry or ch.res_stage == last)),
        "carry_before_residual": bool(ch.carry and ch.res_stage == 0), "res_on_wrong_stage": ch.res_stage >= 0 and nst >= 2,
        "ln_no_clamp": bool(case.hot), "ln_eps_1e-6": case.any_ln, "ln_unbiased_variance": case.any_ln,
        "ln_out_stats_of_neighbour_row": bool(case.ln_out) and case.rows > 1,
        "pool_ceil_grid": bool(case.pool) and (case.pool[1] % 2 == 1 or case.pool[2] % 2 == 1), "pool_sum_not_mean": bool(case.pool),
        "pool_row_stride_of_pooled_grid": bool(case.pool) and case.pool[1] >= 4,
        "tile_rows_from_next_image": case.xcd_tiles > 1,
    }[variant]


def exempt(variant, case):
    """a case the variant's feature applies to but the variant cannot show on it: the rule, or None"""
    if variant == "ln_unbiased_variance" and case.kind == "ensemble":
        return "C - 1 for C scales the normalised row by 1 - 1 / (2 C), 0.1 - 0.4 %: of the size of the ensemble's own 2 D_row; the analytic cases reject it"
    if variant == "ln_eps_1e-6" and (case.rows <= QUIET_ROW or case.ln_rows is None):
        return "no quiet row reaches a LayerNorm: every row's variance is far above eps, or exactly 0 (the constant row normalises to 0 with any eps)"
    if (variant in ("ln_unbiased_variance", "fan_wsum_of_layer0") or (variant == "ln_eps_1e-6" and case.ln_rows == "res")) and case.dtype == F32 \
            and case.nstage + bool(case.nfan) >= 2:
        return "fp32 chains of 2 - 3 stages: the propagated bound is loose by construction (the table shows by how much); the fp16 and one-stage cases reject it"
    if variant == "ln_unbiased_variance" and case.pool:
        return "half an ulp on every pooled input, carried through the LayerNorm and |W|, is wider than 1 / (2 C) of the row"
    if variant == "pool_ceil_grid" and case.pool[0] == 1 and case.pool[1] // 2 == 1:
        return "one image with one pooled row: its first W // 2 entries are the same pixels on the ceil grid"
    if variant == "pool_sum_not_mean" and case.nstage == 0 and case.fan_ln:
        return "a LayerNorm directly on the pooled rows removes the factor 4"
    return None


class Rounder(K13.Rounder):
    """float64 -> the I/O dtype's value (through fp32, as from_f32 rounds), optionally moved to a neighbour.  A value the exact arithmetic
    already lands on is not moved: it arises here only where the kernel's fp32 arithmetic is exact as well (a row of zeros times the weights
    plus a bias that is an I/O-dtype value: the special rows of ln_rows == 'res')."""

    def __init__(self, dtype, seed):
        super().__init__(seed)
        self.dtype = dtype

    def __call__(self, t, exact=False):
        if self.dtype == F16:
            r = super().__call__(t, True)
            return r if (self.g is None or exact) else torch.where(r == t, r, super().__call__(t, False))
        r = _f32(t)
        if self.g is None or exact:
            return r
        u = torch.rand(r.shape, generator=self.g).to(r.device)
        d = (u >= 0.875).double() - (u < 0.125).double()
        d = torch.where((r == 0) | (r == t) | ~torch.isfinite(r), torch.zeros_like(d), d)
        return _f32(r + d * K5.ulp(r, F32))


@functools.lru_cache(maxsize=None)
def half_order(C):
    """(2, C / 2): the channels lane half hi of a wave takes, in order: 16 f + 8 hi + e over the k16 steps f (ln_accumulate on the A fragments)"""
    return torch.tensor([[16 * f + 8 * hi + e for f in range(C // 16) for e in range(8)] for hi in range(2)])


def fold_stats(x, dtype, eps, clamp=True, unbiased=False):
    """mean and rstd of the rows of x as a stage of chain.hip takes them for the fold"""
    C = x.shape[-1]
    if dtype == F16 and not unbiased:
        return K13.ln_stats(x, eps, clamp, order=half_order(C))
    o = half_order(C).to(x.device)
    shift = x[..., :1] if dtype == F32 else torch.zeros_like(x[..., :1])
    d = _f32(x - shift)[..., o]                                                      # (.., 2, C / 2)
    s = torch.zeros(d.shape[:-1], dtype=torch.float64, device=x.device)
    q = torch.zeros_like(s)
    if dtype == F16:                                                                 # (the unbiased variant: pairs as v_dot2 takes them)
        for p in range(o.shape[1] // 2):
            a, b = d[..., 2 * p], d[..., 2 * p + 1]
            s, q = _f32(s + (a + b)), _f32(q + (a * a + b * b))
    else:
        for p in range(o.shape[1]):
            s, q = _f32(s + d[..., p]), _f32(q + d[..., p] * d[..., p])
    s, q = _f32(s.sum(-1)), _f32(q.sum(-1))
    inv = float(np.float32(1.0) / np.float32(C))
    mean = _f32(s * inv)
    var = _f32(_f32(q * inv) - mean * mean)
    if unbiased:
        var = var * C / (C - 1)
    if clamp:
        var = var.clamp(min=0.0)
    rstd = _f32(1.0 / torch.sqrt(_f32(var + float(np.float32(eps)))))
    return _f32(mean[..., None] + shift), rstd[..., None]


def hot_search(C):
    """the first 11-bit constant in [8, 16) whose one-pass variance is negative before the clamp, in the order fold_stats() sums a row of C"""
    cand = torch.arange(1025, 2048).double() / 128.0
    x = cand[:, None].expand(-1, C).contiguous()
    o = half_order(C)
    xs = x[..., o]
    s = torch.zeros(xs.shape[:-1], dtype=torch.float64)
    q = torch.zeros_like(s)
    for p in range(o.shape[1] // 2):
        a, b = xs[..., 2 * p], xs[..., 2 * p + 1]
        s, q = _f32(s + (a + b)), _f32(q + (a * a + b * b))
    s, q = _f32(s.sum(-1)), _f32(q.sum(-1))
    inv = float(np.float32(1.0) / np.float32(C))
    mean = _f32(s * inv)
    var = _f32(_f32(q * inv) - mean * mean)
    neg = torch.nonzero(var < 0).flatten()
    return (float(cand[neg[0]]), float(var[neg[0]])) if neg.numel() else (None, None)


def emulate(case, variant=None, flips=None, device="cpu"):
    """-> (out, ln, fan): (rows, C) / (rows, C) / (rows, nfan C) float64 tensors holding I/O-dtype values, None where the case has no such output"""
    inp, ops, ch = inputs(case, device), _dev_ops(case, device), case.ch
    plain = operands(case)
    C, nst, dt = case.C, case.nstage, case.dtype
    dev = inp.xbuf.device
    rd = Rounder(dt, flips)
    W = list(ops.W)
    fanW = [ops.fanW[f] for f in range(case.nfan)]
    if variant == "k16_halves_swapped":
        perm = torch.arange(C, device=dev).reshape(-1, 2, 8).flip(1).reshape(-1)
        W, fanW = [w[:, perm] for w in W], [w[:, perm] for w in fanW]
    if variant == "frag_tile_stride":
        first = torch.arange(C, device=dev) % 32
        W, fanW = [w[first] for w in W], [w[first] for w in fanW]
    wsum = [wsum_of(w).to(dev) for w in plain.W]
    fanws = [wsum_of(plain.fanW[f]).to(dev) for f in range(case.nfan)]
    zero = torch.zeros(C, dtype=torch.float64, device=dev)
    b = [zero if t is None else t for t in ops.b]
    fanb = [ops.fanb[f * C:(f + 1) * C] if ops.fanb is not None else zero for f in range(case.nfan)]
    eps = 1e-6 if variant == "ln_eps_1e-6" else EPS
    stats = lambda t: fold_stats(t, dt, eps, clamp=variant != "ln_no_clamp", unbiased=variant == "ln_unbiased_variance")   # noqa: E731

    if case.pool:                                                                    # R1
        q = pooled_rows(case, inp, variant)
        ssum = _f32(_f32(_f32(q[0] + q[1]) + q[2]) + q[3])
        x = rd(_f32(ssum * (1.0 if variant == "pool_sum_not_mean" else 0.25)))
    else:
        x = inp.x.double().reshape(case.rows, C)
    res = inp.res.double() if inp.res is not None else None
    rs = ch.res_stage
    if variant == "res_on_wrong_stage":
        rs = (rs + 1) % nst
    t, y0, y0_pre, tile = x, None, None, None
    for s in range(nst):
        Ws = W[s - 1] if (variant == "stage_weights_shifted" and s >= 1) else W[s]
        acc = t @ Ws.T
        if ch.ln[s]:
            mean, rstd = stats(t)
            y = rstd * (acc - mean * wsum[s]) + b[s]
        else:
            y = acc + b[s]
        y = rd(_act64(y, ch.acts[s]))                                                # R2
        tile = y
        last = s == nst - 1
        if not last and s == rs:
            y = rd(y + res, exact=True)                                              # R3
        if s == 0:
            y0, y0_pre = y, tile
        if last:                                                                     # R4: carry, then the residual
            if ch.carry:
                y = rd(y + (y0_pre if variant == "carry_before_residual" else y0), exact=True)
            if s == rs:
                y = rd(y + res, exact=True)
        t = y
    out = t + 0.0 if nst else None
    ln = fan = None
    if case.ln_out:                                                                  # R5
        src = out
        mu = src.mean(-1, keepdim=True)
        rsd = 1.0 / torch.sqrt(((src - mu) ** 2).mean(-1, keepdim=True) + LN_OUT_EPS)
        if variant == "ln_out_stats_of_neighbour_row":
            nb = (torch.arange(case.rows, device=dev) ^ 1).clamp(max=case.rows - 1)
            mu, rsd = mu[nb], rsd[nb]
        ln = rd((out - mu) * rsd * ops.gout + ops.bout)
    if case.nfan:                                                                    # R6
        src = t
        if variant == "fan_reads_unrounded":
            src = tile
        if case.fan_ln:
            mean, rstd = stats(x if variant == "fan_stats_from_input" else src)
        cols = []
        for f in range(case.nfan):
            wf = fanW[0] if variant == "fan_weight_of_layer0" else fanW[f]
            bf = fanb[0] if variant == "fan_bias_of_layer0" else fanb[f]
            acc = src @ wf.T
            if case.fan_ln:
                wsf = fanws[0] if variant == "fan_wsum_of_layer0" else fanws[f]
                cols.append(rd(rstd * (acc - mean * wsf) + bf))
            else:
                cols.append(rd(acc + bf))
        fan = torch.cat(cols, -1) + 0.0
    if variant == "tile_rows_from_next_image":                                       # the tile a block loaded, stored at the block's own index
        bm = case.bm
        src_row = torch.cat([torch.arange(bm) + bm * tile_of_block(case, blk) for blk in range(case.rows // bm)]).to(dev)
        out, ln, fan = (None if o is None else o[src_row] for o in (out, ln, fan))
    return out, ln, fan


def emulate_ln_out_from_unrounded(case, device="cpu"):
    """NOT_SHOWN['ln_out_from_unrounded']: ln_out of the last stage's sum before it is rounded, for a one-stage case with a residual or none"""
    inp, ops = inputs(case, device), _dev_ops(case, device)
    assert case.nstage == 1 and case.ln_out
    rd = Rounder(case.dtype, None)
    x = inp.x.double().reshape(case.rows, case.C)
    y = rd(x @ ops.W[0].T + (ops.b[0] if ops.b[0] is not None else 0.0))
    unr = y + inp.res.double() if case.ch.res_stage == 0 else x @ ops.W[0].T + (ops.b[0] if ops.b[0] is not None else 0.0)
    out = rd(unr)
    return out, rd(_ln64(_f32(unr), LN_OUT_EPS) * ops.gout + ops.bout), None


# ---- bounds and the comparator -------------------------------------------------------------------------------------------------------------
U24 = K5.U24
_Shim = collections.namedtuple("_Shim", "spec dtype K a0 a1")                       # what k5_cases.bound() reads of a case


def half(value, err, dtype):
    return 0.5 * K5.ulp(value.abs() + err, dtype)


def ln_input_bound(t, e, eps=EPS):
    """how far the normalised row moves when the row t moves by at most e per element (ln_out_bound()'s first-order term, factor 1.02)"""
    sig = torch.sqrt(t.var(-1, unbiased=False, keepdim=True) + eps)
    n = (t - t.mean(-1, keepdim=True)) / sig
    return 1.02 * (e + e.mean(-1, keepdim=True) + n.abs() * torch.sqrt((e * e).mean(-1, keepdim=True))) / sig


def stage_bound(case, t, e_in, w, b, ln, act, adds=()):
    """-> (the exact output of one layer on the exact rows t, the elementwise bound of the kernel's I/O-dtype value of it), when the kernel's
    rows are within e_in of t.  adds: (value, its error) of every row tensor added behind the layer, in the kernel's order.  See the docstring."""
    C, dt = case.C, case.dtype
    babs = b.abs() if b is not None else 0.0
    bb = b if b is not None else 0.0
    wa = w.abs()
    if ln:
        ws = wsum_of(w.to(TDT[dt]).cpu()).to(t.device)
        acc, wabs = t @ w.T, t.abs() @ wa.T
        if dt == F32:
            x0 = t[..., :1]
            e = K13.ln_fold_bound(t - x0, (t - x0).abs() @ wa.T, acc - x0 * ws, ws, EPS)
            m = t.mean(-1, keepdim=True)
            rstd = (t.var(-1, unbiased=False, keepdim=True) + EPS) ** -0.5
            e = e + 2 * rstd * ((C + 2) * U24 * wabs + 4 * U24 * (acc.abs() + (m * ws).abs()))
        else:
            e = K13.ln_fold_bound(t, wabs, acc, ws, EPS)
        pre = _ln64(t, EPS) @ w.T + bb
        e = 1.02 * e + U24 * babs + ln_input_bound(t, e_in) @ wa.T
    else:
        pre = t @ w.T + bb
        e = (C + 2) * U24 * ((t.abs() + e_in) @ wa.T + babs) + e_in @ wa.T
    shim = _Shim(K5.Spec(None, None, "gauss", act, 1.0, K5.EPI_NONE, ()), dt, C, None, None)
    e = K5.bound(shim, pre, e / ((C + 2) * U24))                                     # activation and staging on top of the accumulator's error e
    if act == GELU and dt == F32:
        e = e + 0.75e-7 * pre.abs()
    y = _act64(pre, act)
    for a, ea in adds:                                                               # K5's ADD: u |o| and half an ulp of the sum
        y = y + a
        e = e + ea
        e = e + U24 * (y.abs() + e)
        e = e + half(y, e, dt)
    return y, e


def analytic(case, device="cpu"):
    """-> (bound of out, of ln_out, of fan) by stage_bound() layer by layer along the reference's own rows"""
    inp, ops, ch, ref = inputs(case, device), _dev_ops(case, device), case.ch, reference(case, device)
    dt = case.dtype
    e = torch.zeros_like(ref.x)
    if case.pool:
        q = pooled_rows(case, inp)
        e = half(ref.x, 3 * U24 * q.abs().mean(0), dt) + 3 * U24 * q.abs().mean(0)
    res = inp.res.double() if inp.res is not None else None
    zero = lambda v: torch.zeros_like(v)                                            # noqa: E731
    t, e0 = ref.x, None
    for s in range(case.nstage):
        adds = []
        last = s == case.nstage - 1
        if ch.carry and last:
            adds.append((ref.ys[0], e0))
        if s == ch.res_stage:
            adds.append((res, zero(res)))
        y, e = stage_bound(case, t, e, ops.W[s], ops.b[s], ch.ln[s], ch.acts[s], adds)
        assert float((y - ref.ys[s]).abs().max()) <= 1e-9 * max(1.0, float(y.abs().max())), case.id
        if s == 0:
            e0 = e
        t = y
    eo = e if case.nstage else None
    if case.regime == "pass":
        eo = torch.zeros_like(e)                                                     # out is x bit for bit (compare() is given K13.EXACT for it)
    el = ef = None
    if case.ln_out:
        el = ln_out_bound9(case, ref.out, eo, ops.gout, ops.bout)
    if case.nfan:
        cols = []
        for f in range(case.nfan):
            bf = ops.fanb[f * case.C:(f + 1) * case.C] if ops.fanb is not None else None
            cols.append(stage_bound(case, t, e, ops.fanW[f], bf, case.fan_ln, NONE)[1])
        ef = torch.cat(cols, -1)
    if case.regime == "pass":
        eo = torch.full_like(eo, K13.EXACT)
    return eo, el, ef


def ln_out_bound9(case, out, E, g, b):
    """k13_cases.ln_out_bound() plus the rounding it leaves out (found on the pass probe at C = 192, see the docstring): the error of the fp32
    mean itself.  A thread adds the 8 / 4 values of a 16-byte piece (fp16 / fp32) -- of C / 64 pieces on the second-pass path of 24 / 48
    pieces per row -- and the partial sums go through log2(lanes per row) shuffle steps (3 on the second-pass path): every partial sum
    carries at most `depth` roundings, |d sum| <= depth u sum|x|; sum * fl(1 / C) adds 2 u |mean| (nothing when C is a power of two, kept
    for all).  The normalised row moves by d mean / sigma."""
    dt, C = case.dtype, case.C
    vec = 8 if dt == F16 else 4
    ppr = C // vec
    depth = (vec - 1 + int(math.log2(ppr))) if ppr & (ppr - 1) == 0 else (ppr // 8 * vec - 1 + 3)
    sig = torch.sqrt(out.var(-1, unbiased=False, keepdim=True) + LN_OUT_EPS)
    dmean = depth * U24 * (out.abs() + E).mean(-1, keepdim=True) + 2 * U24 * out.mean(-1, keepdim=True).abs()
    return K13.ln_out_bound(out, E, g, b, LN_OUT_EPS, half=lambda v, err: half(v, err, dt)) + 1.02 * g.abs() * dmean / sig


Judge = collections.namedtuple("Judge", "ref bounds members")      # bounds: (out, ln, fan), None entries where there is no such output; exact: all None


@functools.lru_cache(maxsize=4)
def judge(case, device="cpu"):
    ref = reference(case, device)
    refs = (ref.out, ref.ln, ref.fan)
    if case.kind == "exact":                                                         # ln_out of rows the kernel owes exactly: ln_out_bound() with E = 0
        lb = None
        if case.ln_out:
            ops = _dev_ops(case, device)
            lb = ln_out_bound9(case, ref.out, torch.zeros_like(ref.out), ops.gout, ops.bout)
        return Judge(refs, (None, lb, None), [emulate(case, None, None, device)])
    if case.kind == "analytic":
        return Judge(refs, analytic(case, device), [emulate(case, None, None, device)])
    members = [emulate(case, None, None, device)] + [emulate(case, None, sd, device) for sd in FLIP_SEEDS]
    bounds = tuple(None if r is None else K13.token_bound(r, [m[i] for m in members]) for i, r in enumerate(refs))
    return Judge(refs, bounds, members)


def compare(got, ref, bound):
    """every element of one output against the reference: bound None -- the same value and no -0.0; else k13_cases.compare()"""
    if bound is not None:
        return K13.compare(got, ref, bound)
    g = got.detach().double()
    assert g.shape == ref.shape, (g.shape, ref.shape)
    miss = ~(g == ref) | ((g == 0) & torch.signbit(g))
    k = int(miss.double().argmax())
    where = tuple(int(i) for i in torch.unravel_index(torch.tensor(k), miss.shape))
    err = float((g - ref).abs().flatten()[k])
    return K13.Result(err if math.isfinite(err) else float("inf"), 0.0, float("inf") if bool(miss.any()) else 0.0, int(miss.sum()), miss.numel(), where)


WHAT = ("out", "ln", "fan")


def verdict(case, outs, device="cpu"):
    """-> [(what, Result)] of a kernel's (or an emulation's) (out, ln, fan) under the case's bounds"""
    j = judge(case, device)
    return [(WHAT[i], compare(outs[i], j.ref[i], j.bounds[i])) for i in range(3) if j.ref[i] is not None]


def line(case, what, res, sel=None):
    r, c = res.where
    return (f"{case.id:84s} C {case.C:3d} {K5.SHORT[case.dtype]} {sel or case.expected:38s} rows {case.rows:5d} {case.chain:10s} {case.regime:5s} {case.kind:8s} "
            f"{what:3s} max err {res.err:.3e}  bound {res.bound:.3e}  ratio {res.ratio:.3f}  over 1: {res.nbad} of {res.n}  at (row {r}, channel {c})"
            f"  {'ok' if res.ratio <= 1 else 'FAIL'}")


def outside_is_nan(whole, mask):
    """the guard check of the GPU test: every element of the canary outside the output's slice is still NaN"""
    return bool(torch.isnan(whole[~mask]).all())
