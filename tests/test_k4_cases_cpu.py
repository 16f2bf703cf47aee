"""The K4 plan tests without a GPU (tests/k4_cases.py, tests/k4_plans.py; the kernel itself runs in tests/test_hip_k4_plans.py).

Every claimed plan is asked of the launch's own planner (s2m2_attention_plan: host code), and the coverage the case list is there for is
computed on the planner's answers, with the set of reachable plans taken from sweeps of the planner -- no threshold of launch_attn is
restated here.  The float64 reference is held against a plain numpy restatement.  A torch emulation of the kernel's arithmetic passes the
GPU test's comparator under the GPU test's bounds at every case's (Nq, Nk, D), and thirteen wrong variants of it are rejected by every case
they can touch."""
import collections
import ctypes

import numpy as np
import pytest

import k4_cases as K
import k4_plans
from s2m2_amd import hip


@pytest.fixture(scope="module")
def lib():
    from s2m2_amd.build import build
    build(verbose=False)
    return hip.load()


def planned(case, grid="case"):
    p = hip.attention_plan(case.nb, case.heads, case.Nq, case.Nk, case.D, K.TDT[case.dt], case.swap, case.grid if grid == "case" else grid)
    p["lds"] = p.pop("lds_bytes")
    return K.Plan(**p)


def test_every_claimed_plan_is_the_planners(lib):
    wrong = [(c.id, c.plan, planned(c)) for c in K.all_cases() if planned(c) != c.plan]
    assert not wrong, wrong[:5]
    for c in K.all_cases():
        assert c.plan.nw >= c.plan.minw, c.id            # the staging loops are sized for MINW waves


def test_head_dims_without_an_instantiation_are_refused(lib):
    for shape in k4_plans.REFUSED:
        for dt in K.TDT.values():
            with pytest.raises(RuntimeError, match="unsupported head dim"):
                hip.attention_plan(*shape, dt)


def lib_call(nb, heads, Nq, Nk, D, swap, gw, gh, dt, p):
    """the raw entry: its return code instead of an exception (the sweeps ask for shapes the planner refuses)"""
    return hip.load().s2m2_attention_plan(nb, heads, Nq, Nk, D, swap, gw, gh, hip._DT[K.TDT[dt]], ctypes.byref(p))


def _reachable():
    """(dtype, DP, MINW, KSPLIT) -> set of waves per block, over a sweep of the planner (no PE)"""
    reach = collections.defaultdict(set)
    for dt in K.TDT:
        for D in range(8, 385, 8):
            for nb, heads in ((1, 1), (2, 8), (64, 8)):
                for N in list(range(1, 321)) + [512, 992, 1024, 4096]:
                    p = hip.AttnPlan()
                    if lib_call(nb, heads, N, N, D, 0, 0, 0, dt, p) == 0:
                        reach[(dt, p.dp, p.minw, p.ksplit)].add(p.nw)
    return reach


def test_the_case_list_covers_every_reachable_plan(lib):
    reach = _reachable()
    assert len(reach) == 2 * (4 * 3 + 5), sorted(reach)            # d <= 64: MINW 2, MINW 4, key-split; five wide head dims; both dtypes
    plans = {c: planned(c) for c in K.all_cases()}
    by_key = collections.defaultdict(list)
    for c, p in plans.items():
        if c.grid is None:
            by_key[(c.dt, p.dp, p.minw, p.ksplit)].append((c, p))
    for key, nws in sorted(reach.items()):
        got = by_key[key]
        assert {min(nws), max(nws)} <= {p.nw for _, p in got}, (key, sorted(nws), sorted({p.nw for _, p in got}))
        assert any(c.Nq % 32 for c, _ in got), (key, "no ragged last query tile")
        assert any(c.Nk % (32 * p.kt) == 0 for c, p in got), (key, "no Nk at a multiple of the stage")
        assert any(c.Nk % (32 * p.kt) == 1 for c, p in got), (key, "no Nk one past a stage")
        assert any(c.Nk % 32 for c, _ in got), (key, "no partial sub-tile")
    deep = {-(-c.Nk // (32 * p.kt)) for c, p in plans.items() if p.deep}
    assert {1, 2, 3, 4, 5} <= deep, deep
    # PE: every bin tile the planner can choose, and the loop that sheds waves until the tables fit
    tiles = set()
    for gw in range(1, 97):
        for gh in range(1, 97):
            p = hip.AttnPlan()
            if lib_call(1, 1, gw * gh, gw * gh, 16, 0, gw, gh, "float16", p) == 0:
                tiles.add((p.nxt, p.nyt))
    assert len(tiles) == 3 and tiles == {(p.nxt, p.nyt) for c, p in plans.items() if c.grid}
    assert any(c.grid and not p.ksplit and p.nw < planned(c, grid=None).nw for c, p in plans.items()), "no PE case sheds waves"
    # both sides of both key-split thresholds: neighbours in the number of query tiles, and in Nk, that differ in the mode
    ntq = lambda c: -(-c.Nq // 32)
    same = lambda a, b: (a.nb, a.heads, a.D, a.dt, a.grid, a.swap) == (b.nb, b.heads, b.D, b.dt, b.grid, b.swap)
    flat = [(c, p) for c, p in plans.items() if c.grid is None]
    for dt in K.TDT:
        assert any(same(a, b) and a.dt == dt and ntq(a) == ntq(b) + 1 and not pa.ksplit and pb.ksplit for a, pa in flat for b, pb in flat), dt
        assert any(same(a, b) and a.dt == dt and a.Nk + 1 == b.Nk and ntq(a) == ntq(b) and not pa.ksplit and pb.ksplit
                   for a, pa in flat for b, pb in flat), dt


def test_block_counts_that_are_no_multiple_of_8(lib):
    counts = {c.plan.nblk * c.nb * c.heads for c in K.all_cases()}
    assert {1, 3, 7, 9} <= counts


def _numpy_reference(case):
    inp = K.inputs(case)
    nb, heads, Nq, Nk, D = case.shape
    q, k, v = (t.double().numpy().reshape(nb, -1, heads, D) for t in (inp.q, inp.k, inp.v))
    out = np.zeros((nb, Nq, heads, D))
    pe = np.zeros((nb, Nq, heads, 32))
    for b in range(nb):
        bk = K.bkv(case, b)
        for h in range(heads):
            for i in range(Nq):
                s = np.array([np.dot(q[b, i, h], k[bk, j, h]) for j in range(Nk)]) * case.scale
                w = np.exp(s - s.max())
                w /= w.sum()
                out[b, i, h] = sum(w[j] * v[bk, j, h] for j in range(Nk))
                if case.grid:
                    gw, gh = case.grid
                    px, py = inp.px.double().numpy(), inp.py.double().numpy()
                    for j in range(Nk):
                        pe[b, i, h, :16] += w[j] * 0.5 * px[i % gw - j % gw + gw - 1]
                        pe[b, i, h, 16:] += w[j] * 0.5 * py[i // gw - j // gw + gh - 1]
    return out.reshape(nb, Nq, -1), pe.reshape(nb, Nq, -1)


@pytest.mark.parametrize("key", [(2, 2, 8, 100, 64, False, None), (4, 2, 130, 130, 88, True, None), (2, 8, 24, 24, 32, False, (8, 3))], ids=str)
def test_reference_against_numpy(key):
    case = [c for c in K.all_cases() if c[:5] + (c.swap, c.grid) == key and c.dt == "float16"][0].small()
    if case.Nq > 40:
        case = case._replace(Nq=9, Nk=40)            # (the swap case, cut to a size plain loops manage; swap needs Nq == Nk only at the launch)
    ref = K.reference(case)
    out, pe = _numpy_reference(case)
    assert np.abs(ref.out.numpy() - out).max() < 1e-12
    if case.grid:
        assert np.abs(ref.pe.numpy() - pe).max() < 1e-12
    assert bool((ref.bound > 0).all())


def _small_cases():
    seen = {}
    for c in K.all_cases():
        seen.setdefault(c.small(), c)
    return list(seen)


def _ratio(case, ref, got):
    out, pe = got if case.grid else (got, None)
    r = K.compare(out, ref.out, ref.bound)
    rp = K.compare(pe, ref.pe, ref.pe_bound) if case.grid else None
    return r, rp


@pytest.mark.parametrize("case", _small_cases(), ids=lambda c: c.id)
def test_emulation_passes_and_every_wrong_variant_is_rejected(case):
    ref = K.reference(case)
    r, rp = _ratio(case, ref, K.emulate(case))
    assert r.ratio <= 1, K.line(case, r)
    assert rp is None or rp.ratio <= 1, K.line(case, rp, "pe")
    for variant in K.VARIANTS:
        if not K.applies(variant, case) or K.exempt(variant, case):
            continue
        r, rp = _ratio(case, ref, K.emulate(case, variant))
        worst = rp.ratio if variant.startswith("pe_") else max(r.ratio, rp.ratio if rp else 0.0)
        assert worst > 1, f"{variant} passes: {K.line(case, rp if variant.startswith('pe_') else r)}"


def test_exemptions_stay_within_a_quarter():
    for variant in K.VARIANTS:
        smalls = [c.small() for c in K.all_cases()]
        app = [c for c in smalls if K.applies(variant, c)]
        ex = [c for c in app if K.exempt(variant, c)]
        assert app, variant
        assert 4 * len(ex) <= len(app), (variant, len(ex), len(app))


def test_key_row_by_reciprocal_is_exact():
    """(int)(((float)kv + 0.5f) * (1.0f / gw)) of the PE one-hot operands is kv / gw on every grid the kernel is instantiated for"""
    f = np.float32
    kv = np.arange(96 * 96)
    for gw in range(1, 97):
        inv = f(1.0) / f(gw)
        y = ((kv.astype(f) + f(0.5)) * inv).astype(np.int32)
        assert y.dtype == np.int32 and (kv.astype(f) * inv).dtype == f
        assert np.array_equal(y, kv // gw), gw
