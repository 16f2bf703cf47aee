"""K4 (s2m2_attention, csrc/attention.hip) through the raw C entry against a float64 reference, on every launch plan its planner produces.

The cases (tests/k4_cases.py, tests/k4_plans.py) reach every head-dim instantiation with the fewest and the most waves it is launched with, the
key-split mode with one to ten stages (one to five of the 256-key stages of the fp16 pipeline), the two-sweep softmax, queries in LDS, every
positional-encoding bin tile and the loop that sheds waves, Nq != Nk in both directions, and both sides of the dispatch thresholds;
tests/test_k4_cases_cpu.py holds each case to the plan the planner reports and shows that the comparator used here rejects thirteen wrong
variants of the kernel's arithmetic.

Every case: q, k, v are channel slices of one row buffer with guard rows of large finite values around the tokens (a read past Nk of the
last batch changes the result and stays inside the allocation); ``out`` (and ``pe_out``) is a channel slice of a wider NaN-filled tensor with
NaN rows before and after.  Every element inside is compared with the float64 reference, evaluated on the device, under the elementwise
bounds of k4_cases.py (a NaN left inside has ratio inf); every element outside must still be NaN.  The 19 shapes of
tests/test_hip_attention.py go through the same comparator.  Four launches of a key-split and of a two-sweep case are bit-identical.
S2M2_K4_PLANS_TABLE=<path> appends one line per case: plan, worst error, its bound, their ratio, element (profiles/k4/k4_plans.txt)."""
import ctypes
import os

import pytest
import torch

import k4_cases as K

pytestmark = pytest.mark.gpu
TABLE = []
DEV = "cuda"
PAD = 8                  # NaN channels on either side of out / pe_out


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    path = os.environ.get("S2M2_K4_PLANS_TABLE")
    if path and TABLE:
        with open(path, "a") as f:
            f.write("\n".join(TABLE) + "\n")


def canary(rows, width, dtype):
    """(whole NaN tensor, the (rows, width) slice in its middle, mask of the slice)"""
    whole = torch.full((rows + 2, width + 2 * PAD), float("nan"), device=DEV, dtype=dtype)
    mask = torch.zeros_like(whole, dtype=torch.bool)
    mask[1:-1, PAD:PAD + width] = True
    return whole, whole[1:-1, PAD:PAD + width], mask


def launch(hip, case, inp):
    """-> (out, pe_out or None) as (nb, Nq, .) views of their NaN canaries, after the canaries were checked"""
    nb, heads, Nq, Nk, D = case.shape
    dt = K.TDT[case.dt]
    W = inp.buf.shape[1]
    assert inp.q.stride(1) == inp.k.stride(1) == inp.v.stride(1) == W
    whole, out, mask = canary(nb * Nq, case.C, dt)
    gw, gh = case.grid or (0, 0)
    pw = pout = pmask = None
    if case.grid:
        pw, pout, pmask = canary(nb * Nq, heads * 32, dt)
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = hip.load().s2m2_attention(vp(inp.q), vp(inp.k), vp(inp.v), vp(out), W, W, W, whole.shape[1], nb, heads, Nq, Nk, D, case.scale,
                                   int(case.swap), vp(inp.px), vp(inp.py), vp(pout), pw.shape[1] if case.grid else 0, gw, gh, hip._DT[dt],
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, hip.load().s2m2_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(whole[~mask]).all()), "written outside out"
    if case.grid:
        assert bool(torch.isnan(pw[~pmask]).all()), "written outside pe_out"
    return out.reshape(nb, Nq, -1), pout.reshape(nb, Nq, -1) if case.grid else None


def check(hip, case):
    inp = K.inputs(case, DEV)
    guard = inp.buf.clone()
    ref = K.reference(case, DEV)
    out, pe = launch(hip, case, inp)
    assert torch.equal(inp.buf, guard), "the inputs were written"
    res = K.compare(out, ref.out, ref.bound)
    TABLE.append(K.line(case, res))
    print(TABLE[-1])
    assert res.ratio <= 1, K.line(case, res)
    if case.grid:
        rp = K.compare(pe, ref.pe, ref.pe_bound)
        TABLE.append(K.line(case, rp, "pe"))
        print(TABLE[-1])
        assert rp.ratio <= 1, K.line(case, rp, "pe")


@pytest.mark.parametrize("case", K.all_cases(), ids=lambda c: c.id)
def test_every_plan_vs_float64(hip, case):
    check(hip, case)


# the non-PE shapes of tests/test_hip_attention.py: nb, heads, N, D, swap
EXISTING = [
    (6, 1, 304, 128, False), (4, 1, 304, 128, True), (4, 2, 152, 64, True), (4, 4, 76, 64, False), (2, 8, 300, 32, False),
    (2, 8, 1216, 32, True), (1, 8, 300, 16, False), (3, 1, 8, 128, False), (2, 1, 33, 64, True), (2, 2, 95, 48, False),
    (2, 1, 70, 256, True), (2, 2, 65, 96, False), (1, 8, 100, 24, False),
    (2, 1, 304, 192, False), (2, 1, 70, 192, True), (2, 1, 304, 256, False), (2, 1, 608, 384, False), (4, 1, 100, 384, True), (1, 1, 8, 384, False),
]


@pytest.mark.parametrize("dt", ["float32", "float16"])
@pytest.mark.parametrize("shape", EXISTING, ids=str)
def test_shapes_of_test_hip_attention_vs_float64(hip, shape, dt):
    nb, heads, N, D, swap = shape
    p = hip.attention_plan(nb, heads, N, N, D, K.TDT[dt], swap)
    p["lds"] = p.pop("lds_bytes")
    check(hip, K.Case(nb, heads, N, N, D, dt, swap, None, K.Plan(**p)))


@pytest.mark.parametrize("key", [((2, 8, 1216, 1216, 32), "float16"), ((2, 1, 304, 304, 192), "float16"), ((2, 1, 304, 304, 384), "float32")], ids=str)
def test_four_launches_are_bit_identical(hip, key):
    case = [c for c in K.all_cases() if c.shape == key[0] and c.dt == key[1] and not c.grid][0]
    assert case.plan.deep or case.plan.twopass
    inp = K.inputs(case, DEV)
    first, _ = launch(hip, case, inp)
    for _ in range(3):
        again, _ = launch(hip, case, inp)
        assert torch.equal(again, first)
