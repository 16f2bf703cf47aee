"""K9 (s2m2_mlp_chain, csrc/chain.hip) through the raw C entry against a float64 reference, on every form, tile height and width.

The cases (tests/k9_cases.py) reach the staged form in fp16 and fp32, the direct form and the fan-out-only form at every width and tile height
the host selector can choose (the tall tiles by row count: one and 37 rows in the last tile, and exactly the threshold, which must take the
32-row tile), one to three stages, one to four fan-out layers, the pooled tile load on even and odd grids, the XCD placement with one and two
tiles per group, and every stride at a non-minimal value; tests/test_k9_cases_cpu.py holds that coverage and shows that the comparator used
here rejects eighteen wrong variants of the kernel.

Every case: x and res are channel slices of wider buffers of large finite guard values with a guard row (image) before and after; out, ln_out
and fan_out are channel slices of NaN tensors with NaN rows before and after.  Every element inside is judged by k9_cases.compare() under the
case's bound -- equality of bits in the exact regime, the analytic elementwise bound of the one-stage, fan-out-only and fp32 cases, the per-row
bound ulp16(max(1, |R|)) + 2 D_row of the fp16 chains -- and a NaN left inside has ratio inf; every element outside must still be NaN (a
ragged last tile that stores one row too many lands there); inputs, weights and vectors must be unchanged bit for bit.  The form the host
selector prints for the descriptor must be the one the case is meant for.  Four launches of a direct and a fan-out-only case of every width
are bit-identical.  A placement hint that is no tile multiple gives the bits of no hint.  What the entry must refuse, it refuses without
launching.  S2M2_K9_TABLE=<path> appends one line per case and output: C, dtype, the selected form / BM / NW, rows, chain, regime, worst
error, its bound, their ratio, the element (profiles/k9/k9_chain.txt)."""
import collections
import ctypes
import os

import pytest
import torch

import k9_cases as K

pytestmark = pytest.mark.gpu
TABLE = []
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    path = os.environ.get("S2M2_K9_TABLE")
    if path and TABLE:
        with open(path, "a") as f:
            f.write("\n".join(TABLE) + "\n")


def canary(rows, stride, width, dtype):
    """(whole NaN tensor, its (rows, width) slice, mask of the slice): one NaN row before and after, NaN channels around where the stride has room"""
    pad = K.pad_of(stride, width)
    whole = torch.full((rows + 2, stride), float("nan"), device=DEV, dtype=K.TDT[dtype])
    mask = torch.zeros_like(whole, dtype=torch.bool)
    mask[1:-1, pad:pad + width] = True
    return whole, whole[1:-1, pad:pad + width], mask


Run = collections.namedtuple("Run", "d outs canaries keep")


def bits(t):
    return t.contiguous().view(torch.uint8)


def prepare(hip, case, inp, pk):
    """the descriptor of a case with fresh NaN canaries -> Run(descriptor, (out, ln, fan) views, [(name, whole, mask)], what must stay alive)"""
    C, ch = case.C, case.ch
    d = hip.ChainDesc()
    d.x, d.x_stride, d.rows, d.C, d.dtype, d.nstage = inp.x.data_ptr(), case.xs, case.rows, C, hip._DT[K.TDT[case.dtype]], case.nstage
    assert inp.x.stride(-2) == case.xs and inp.x.data_ptr() % 16 == 0
    if case.pool:
        d.pool_h, d.pool_w = case.pool[1], case.pool[2]
    for s in range(case.nstage):
        d.weight[s], d.act[s] = pk.W[s].data_ptr(), ch.acts[s]
        d.bias[s] = pk.b[s].data_ptr() if pk.b[s] is not None else None
        d.ln_wsum[s] = pk.wsum[s].data_ptr() if ch.ln[s] else None
    d.res_stage, d.carry, d.ln_eps, d.weight_frag, d.xcd_group_rows = ch.res_stage, ch.carry, K.EPS, int(case.frag), case.xcd
    if ch.res_stage >= 0:
        d.res, d.res_stride = inp.res.data_ptr(), case.rs
        assert inp.res.stride(0) == case.rs
    outs, canaries = [None, None, None], []
    if case.nstage:
        whole, out, mask = canary(case.rows, case.os, C, case.dtype)
        d.out, d.out_stride = out.data_ptr(), case.os
        outs[0] = out
        canaries.append(("out", whole, mask))
    if case.ln_out:
        whole, ln, mask = canary(case.rows, case.ls, C, case.dtype)
        d.ln_out, d.ln_out_stride, d.ln_gamma, d.ln_beta, d.ln_out_eps = ln.data_ptr(), case.ls, pk.gout.data_ptr(), pk.bout.data_ptr(), K.LN_OUT_EPS
        outs[1] = ln
        canaries.append(("ln_out", whole, mask))
    if case.nfan:
        whole, fan, mask = canary(case.rows, case.fs, case.nfan * C, case.dtype)
        d.fan_weight, d.fan_out, d.fan_out_stride, d.nfan = pk.fanW.data_ptr(), fan.data_ptr(), case.fs, case.nfan
        d.fan_bias = pk.fanb.data_ptr() if pk.fanb is not None else None
        d.fan_ln_wsum = pk.fanwsum.data_ptr() if case.fan_ln else None
        outs[2] = fan
        canaries.append(("fan_out", whole, mask))
    return Run(d, tuple(outs), canaries, (inp, pk))


def launch(hip, case, inp, pk, change=None):
    """-> (out, ln, fan) views of their NaN canaries, after the canaries were checked"""
    run = prepare(hip, case, inp, pk)
    if change:
        change(run.d)
    rc = hip.load().s2m2_mlp_chain(ctypes.byref(run.d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, hip.load().s2m2_last_error().decode()
    torch.cuda.synchronize()
    for name, whole, mask in run.canaries:
        assert K.outside_is_nan(whole, mask), f"written outside {name}"
    return run.outs


def _tensors(inp, pk):
    ts = [inp.xbuf, inp.rbuf, pk.fanW, pk.fanb, pk.fanwsum, pk.gout, pk.bout] + list(pk.W) + list(pk.b) + list(pk.wsum)
    return [t for t in ts if t is not None]


def check(hip, case):
    sel = K.chosen(case)
    assert sel == case.expected, (case.id, sel, case.expected)
    inp, pk = K.inputs(case, DEV), K.packed(case, DEV)
    before = [t.clone() for t in _tensors(inp, pk)]
    outs = launch(hip, case, inp, pk)
    for t, b in zip(_tensors(inp, pk), before):
        assert torch.equal(bits(t), bits(b)), "an input, a weight or a vector was written"
    bad = []
    for what, res in K.verdict(case, outs, DEV):
        TABLE.append(K.line(case, what, res, sel))
        print(TABLE[-1])
        if not res.ratio <= 1:
            bad.append(TABLE[-1])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", K.all_cases(), ids=lambda c: c.id)
def test_every_form_vs_float64(hip, case):
    check(hip, case)


def _one_per_width(form):
    seen = {}
    for c in K.all_cases():
        if c.form == form and c.regime == "gauss" and c.rows >= 31 and c.bm == 32 and not c.pool:
            seen.setdefault(c.C, c)
    assert set(seen) == {128, 192, 256, 384, 512}
    return list(seen.values())


@pytest.mark.parametrize("case", _one_per_width("direct") + _one_per_width("fan_only"), ids=lambda c: c.id)
def test_four_launches_are_bit_identical(hip, case):
    """the direct and the fan-out-only form have no barrier inside a stage"""
    inp, pk = K.inputs(case, DEV), K.packed(case, DEV)
    first = [None if o is None else o.clone() for o in launch(hip, case, inp, pk)]
    for _ in range(3):
        for a, b in zip(launch(hip, case, inp, pk), first):
            assert a is None or torch.equal(bits(a), bits(b))


def test_a_hint_that_is_no_tile_multiple_is_ignored(hip):
    case = next(c for c in K.all_cases() if c.xcd == 48)
    assert case.xcd_tiles == 0 and K.chosen(case).endswith("xcd=0")
    inp, pk = K.inputs(case, DEV), K.packed(case, DEV)
    hinted = [None if o is None else o.clone() for o in launch(hip, case, inp, pk)]
    plain = launch(hip, case, inp, pk, change=lambda d: setattr(d, "xcd_group_rows", 0))
    for a, b in zip(hinted, plain):
        assert a is None or torch.equal(bits(a), bits(b))


def _base(kind):
    cs = K.all_cases()
    if kind == "chain":
        return next(c for c in cs if c.form == "staged" and c.C == 128 and c.dtype == K.F16 and c.chain == "attn_tail" and c.regime == "gauss" and c.nfan == 3)
    if kind == "two":
        return next(c for c in cs if c.form == "staged" and c.C == 128 and c.dtype == K.F16 and c.chain == "conv1x1" and c.regime == "gauss")
    if kind == "ln":
        return next(c for c in cs if c.form == "staged" and c.C == 128 and c.dtype == K.F16 and c.chain == "norm_only" and c.regime == "gauss")
    if kind == "f32":
        return next(c for c in cs if c.dtype == K.F32 and c.C == 128 and c.chain == "plain1")
    if kind == "pool":
        return next(c for c in cs if c.chain == "pooled" and c.regime == "gauss" and c.pool == (2, 8, 18))
    if kind == "poolfan":
        return next(c for c in cs if c.chain == "fan" and c.regime == "gauss" and c.pool == (2, 8, 18))
    return next(c for c in cs if c.form == "fan_only" and c.regime == "gauss" and not c.pool and c.bm == 32 and c.rows >= 31)


def _set(**kw):
    def change(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return change


def _act3(d):
    d.act[0] = 3


def _res_from_x(**kw):
    def change(d):
        d.res, d.res_stride = d.x, d.x_stride
        _set(**kw)(d)
    return change


def _ln_from_out(d):
    d.ln_out, d.ln_out_stride, d.ln_gamma, d.ln_beta, d.ln_out_eps = d.fan_out, d.fan_out_stride, d.fan_weight, d.fan_weight, 1e-5


REFUSALS = [
    ("C=192 staged", "chain", _set(C=192), "not supported"), ("C=640", "chain", _set(C=640), "not supported"),
    ("fp32 C=512", "f32", _set(C=512), "not supported"), ("weight_frag with fp32", "f32", _set(weight_frag=1), "weight_frag"),
    ("x_stride below C", "chain", _set(x_stride=120), "row strides"), ("x_stride 132", "chain", _set(x_stride=132), "row strides"),
    ("out_stride below C", "chain", _set(out_stride=120), "row strides"), ("out_stride 132", "chain", _set(out_stride=132), "row strides"),
    ("res_stride below C", "chain", _set(res_stride=120), "res_stage needs"), ("res_stride 132", "chain", _set(res_stride=132), "res_stage needs"),
    ("fan_out_stride below 3 C", "chain", _set(fan_out_stride=376), "fan-out stages need"), ("fan_out_stride 388", "chain", _set(fan_out_stride=388), "fan-out stages need"),
    ("ln_out_stride below C", "ln", _set(ln_out_stride=120), "ln_out needs"), ("ln_out_stride 132", "ln", _set(ln_out_stride=132), "ln_out needs"),
    ("ln_out with eps 0", "ln", _set(ln_out_eps=0.0), "ln_out needs"),
    ("carry with two stages", "two", _set(carry=1), "carry"), ("res_stage 2 of two stages", "two", _res_from_x(res_stage=2), "res_stage=2"),
    ("res_stage 3 of three", "chain", _set(res_stage=3), "res_stage=3"), ("act 3", "chain", _act3, "act[0]=3"),
    ("nfan 5", "chain", _set(nfan=5), "nfan=5"), ("nfan 5, fan-out only", "fan", _set(nfan=5), "nfan=5"),
    ("pooling without weight_frag", "pool", _set(weight_frag=0), "pool_h"), ("rows not the pooled grid", "pool", _set(rows=71), "pool_h"),
    ("pooling with res", "pool", _res_from_x(res_stage=0), "pooled tile load"), ("pooling with the hint", "pool", _set(xcd_group_rows=9), "pooled tile load"),
    ("pooling with ln_out", "pool", _ln_from_out, "pooled tile load"), ("pooled fan-out only with the hint", "poolfan", _set(xcd_group_rows=9), "pooled tile load"),
    ("nstage 0 without weight_frag", "fan", _set(weight_frag=0), "fan-out only (nstage = 0) exists"),
    ("fan-out only with res_stage", "fan", _res_from_x(res_stage=0), "fan-out-only launch"), ("fan-out only with carry", "fan", _set(carry=1), "fan-out-only launch"),
    ("fan-out only with ln_out", "fan", _ln_from_out, "fan-out-only launch"), ("fan-out only with the hint", "fan", _set(xcd_group_rows=32), "fan-out-only launch"),
]


@pytest.mark.parametrize("ref", REFUSALS, ids=lambda r: r[0])
def test_refusals(hip, ref):
    """the entry returns non-zero, s2m2_last_error names the reason, and nothing is launched: the outputs stay NaN, the inputs as they were"""
    name, kind, change, reason = ref
    case = _base(kind)
    inp, pk = K.inputs(case, DEV), K.packed(case, DEV)
    before = [t.clone() for t in _tensors(inp, pk)]
    run = prepare(hip, case, inp, pk)
    change(run.d)
    rc = hip.load().s2m2_mlp_chain(ctypes.byref(run.d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0, name
    msg = hip.load().s2m2_last_error().decode()
    assert "mlp_chain" in msg and reason in msg, (name, msg)
    for what, whole, _ in run.canaries:
        assert bool(torch.isnan(whole).all()), (name, what)
    for t, b in zip(_tensors(inp, pk), before):
        assert torch.equal(bits(t), bits(b)), name
