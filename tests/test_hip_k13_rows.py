"""K13 (s2m2_row_attn, csrc/rowattn.hip) through the raw C entry against a float64 reference, token by token, at every wave count.

The cases (tests/k13_cases.py) reach one to ten waves, both thread instantiations on either side of 160 | 161 tokens, one and two key chunks
(the second chunk of a single key included), full and one-token last tiles, heads 1 and 2, cross and self attention with 1 to 6 images, the
XCD placement on and off, x strides 128 / 136 / 260, out strides 128 / 132 and ln_out stride 140; tests/test_k13_cases_cpu.py holds that
coverage, and shows that the comparator used here rejects nineteen wrong variants of the kernel.

Every case: x is a channel slice of a wider buffer of large finite guard values (a read outside the tokens changes a result and stays inside
the allocation); out and ln_out are channel slices of NaN tensors with NaN rows before and after.  Every element inside is judged by
k13_cases.compare() under the case's bound -- the per-token bound ulp16(max(1, |R|)) + 2 D_t of the full regime, the analytic bounds of the
route and probe regimes -- and a NaN left inside has ratio inf; every element outside must still be NaN; x must be unchanged bit for bit.  The eleven
shapes of tests/test_hip_rowattn.py go through the same comparator.  Four launches of a two-chunk case of each head count and of the
one-key second chunk are bit-identical.  What the entry must refuse, it refuses without launching.
S2M2_K13_TABLE=<path> appends one line per case and output: w, waves, chunks, regime, worst error, its bound, their ratio, the element
(profiles/k13/k13_rows.txt)."""
import ctypes
import os

import pytest
import torch

import k13_cases as K

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
    path = os.environ.get("S2M2_K13_TABLE")
    if path and TABLE:
        with open(path, "a") as f:
            f.write("\n".join(TABLE) + "\n")


def canary(rows, stride):
    """(whole NaN tensor, its (rows, 128) slice, mask of the slice): one NaN row before and after, NaN channels around where the stride has room"""
    pad = (stride - K.C) // 8 * 4
    whole = torch.full((rows + 2, stride), float("nan"), device=DEV, dtype=torch.float16)
    mask = torch.zeros_like(whole, dtype=torch.bool)
    mask[1:-1, pad:pad + K.C] = True
    return whole, whole[1:-1, pad:pad + K.C], mask


def descriptor(hip, case, inp, wts, vec, out, ln):
    d = hip.RowAttnDesc()
    d.x, d.x_stride, d.out, d.out_stride = inp.x.data_ptr(), case.xs, out.data_ptr(), case.os
    d.nimg, d.h, d.w, d.C, d.heads, d.cross = case.nimg, case.h, case.w, K.C, case.heads, int(case.cross)
    d.weights, d.vectors, d.ln_eps, d.dtype = wts.data_ptr(), vec.data_ptr(), K.EPS, hip._DT[torch.float16]
    d.xcd_hint = int(case.xcd)
    if ln is not None:
        d.ln_out, d.ln_out_stride, d.ln_out_eps = ln.data_ptr(), case.ls, K.LN_OUT_EPS
    return d


def launch(hip, case, inp, packed):
    """-> (out, ln or None) as (rows, w, 128) views of their NaN canaries, after the canaries were checked"""
    n = case.rows * case.w
    assert inp.x.data_ptr() == inp.buf.data_ptr() + 2 * inp.base and inp.x.stride(1) == case.xs
    whole, out, mask = canary(n, case.os)
    lw = ln = lmask = None
    if case.ln_out:
        lw, ln, lmask = canary(n, case.ls)
    d = descriptor(hip, case, inp, packed[0], packed[1], out, ln)
    rc = hip.load().s2m2_row_attn(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, hip.load().s2m2_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(whole[~mask]).all()), "written outside out"
    if case.ln_out:
        assert bool(torch.isnan(lw[~lmask]).all()), "written outside ln_out"
    view = lambda t: t.reshape(case.rows, case.w, K.C)                               # noqa: E731
    return view(out), view(ln) if case.ln_out else None


def check(hip, case):
    inp = K.inputs(case, DEV)
    guard = inp.buf.clone()
    packed = K.packed(K.ops_of(case), DEV)
    out, ln = launch(hip, case, inp, packed)
    assert torch.equal(inp.buf, guard), "the inputs were written"
    bad = []
    for what, res in K.verdict(case, out, ln, DEV):
        TABLE.append(K.line(case, what, res))
        print(TABLE[-1])
        if not res.ratio <= 1:
            bad.append(TABLE[-1])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", K.all_cases(), ids=lambda c: c.id)
def test_every_width_vs_float64(hip, case):
    check(hip, case)


# the shapes of tests/test_hip_rowattn.py: nimg, h, w, heads, cross, ln_out
EXISTING = [(2, 8, 304, 1, True, False), (2, 8, 304, 1, False, True), (2, 16, 160, 1, True, True), (2, 8, 152, 2, True, False), (2, 8, 152, 2, False, False),
            (4, 3, 300, 1, True, False), (2, 5, 76, 2, True, True), (2, 4, 40, 1, False, False), (2, 2, 320, 2, True, False), (6, 2, 24, 1, True, False),
            (2, 24, 200, 1, True, True)]


@pytest.mark.parametrize("shape", EXISTING, ids=str)
def test_shapes_of_test_hip_rowattn_vs_float64(hip, shape):
    check(hip, K.existing_case(*shape))


@pytest.mark.parametrize("key", [(288, 1), (288, 2), (161, 1), (161, 2)], ids=str)
def test_four_launches_are_bit_identical(hip, key):
    case = next(c for c in K.all_cases() if (c.w, c.heads) == key and c.regime == "full")
    assert case.nchunk == 2
    inp, packed = K.inputs(case, DEV), K.packed(K.ops_of(case), DEV)
    first = launch(hip, case, inp, packed)
    for _ in range(3):
        again = launch(hip, case, inp, packed)
        assert torch.equal(again[0], first[0])
        assert first[1] is None or torch.equal(again[1], first[1])


def _mutations():
    def setw(w):
        return lambda d, t: setattr(d, "w", w)

    def x_is_out(d, t):
        d.out = d.x

    def off8(d, t):
        d.weights = d.weights + 8

    def ln_eps0(d, t):
        d.ln_out_eps = 0.0
    return [("w=7", setw(7), False, "w="), ("w=321", setw(321), False, "w="),
            ("odd nimg with cross", lambda d, t: setattr(d, "nimg", 3), False, "even number"),
            ("x == out", x_is_out, False, "distinct"),
            ("x_stride 127", lambda d, t: setattr(d, "x_stride", 127), False, "strides"), ("x_stride 130", lambda d, t: setattr(d, "x_stride", 130), False, "strides"),
            ("out_stride 127", lambda d, t: setattr(d, "out_stride", 127), False, "strides"), ("out_stride 130", lambda d, t: setattr(d, "out_stride", 130), False, "strides"),
            ("weights off by 8 bytes", off8, False, "aligned"),
            ("ln_eps 0", lambda d, t: setattr(d, "ln_eps", 0.0), False, "ln_eps"),
            ("ln_out with eps 0", ln_eps0, True, "ln_out"),
            ("ln_out stride 127", lambda d, t: setattr(d, "ln_out_stride", 127), True, "ln_out"),
            ("ln_out stride 130", lambda d, t: setattr(d, "ln_out_stride", 130), True, "ln_out")]


@pytest.mark.parametrize("mut", _mutations(), ids=lambda m: m[0])
def test_refusals(hip, mut):
    """the entry returns non-zero, s2m2_last_error names the reason, and nothing is launched: out and ln_out stay NaN"""
    name, change, want_ln, reason = mut
    case = next(c for c in K.all_cases() if c.cross and c.nimg == 4 and c.ln_out == want_ln and c.rows <= 16)
    inp, (wts, vec) = K.inputs(case, DEV), K.packed(K.ops_of(case), DEV)
    n = case.rows * case.w
    whole, out, _ = canary(n, case.os)
    lw, ln, _ = canary(n, case.ls) if want_ln else (None, None, None)
    guard = inp.buf.clone()
    d = descriptor(hip, case, inp, wts, vec, out, ln)
    change(d, None)
    rc = hip.load().s2m2_row_attn(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0, name
    msg = hip.load().s2m2_last_error().decode()
    assert "row_attn" in msg and reason in msg, (name, msg)
    assert bool(torch.isnan(whole).all()) and (lw is None or bool(torch.isnan(lw).all())), name
    assert torch.equal(inp.buf, guard)
