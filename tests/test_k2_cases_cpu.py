"""The inputs of tests/test_hip_k2_edges.py are what they claim to be (CPU, no kernel): tests/k2_cases.py builds token-like cost volumes and
their float64 reference; here every case of the GPU test is checked for the properties the GPU asserts lean on, the fp32 oracle is run
through the GPU test's own comparator (k2_cases.check) -- it must pass -- and so are a few deliberately wrong variants, which must not.
The dispatch classes the GPU test's header names are recomputed from the restated LDS formula."""
import pytest
import torch

import k2_cases as K

CASES = [(w, pos, dt, 2, 1, 3) for w in K.WIDTHS for dt in ("float32", "float16") for pos in (True, False)]
CASES.append((136, True, "float16", 3, 2, 3))
CASES += [(w, pos, "float16" if pos else "float32", 2, 1, it) for w, pos in ((136, True), (304, True), (520, False)) for it in (1, 2, 5)]
CASES += [(w, True, dt, 2, 1, 3) for w in (16, 136, 304) for dt in ("float32", "float16") if (w, True, dt, 2, 1, 3) not in CASES]


def _id(c):
    w, pos, dt, h, B, it = c
    return f"w{w}-{K.SHORT[dt]}-pos{int(pos)}-h{h}-B{B}-it{it}"


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_case_is_token_like_and_the_fp32_oracle_passes(c):
    w, pos, dt, h, B, it = c
    case = K.build(w, pos, dt, h, B)
    ref = K.reference(w, pos, dt, h, B, it)
    assert ref.disp.dtype == torch.float64 and ref.conf.dtype == torch.float64 and ref.occ.dtype == torch.float64
    if dt == "float16":
        assert torch.equal(case.cv, case.cv.half().float())
    assert K.column_range(case.cv, pos) > 100
    assert case.planted and all(y < h and 0 <= j <= i < w for y, i, j in case.planted)
    for y, i, j in case.planted:
        assert bool(ref.sure[:, y, i].all()), f"planted pixel ({y}, {i}) is not sure"
        assert bool((ref.ind[:, y, i] == j).all()), f"planted pixel ({y}, {i}) -> {ref.ind[:, y, i].tolist()}, not {j}"
    assert float((~ref.sure).double().mean()) <= K.NOT_SURE_CAP
    assert float(ref.occ.min()) < 0.05, "no row for the dustbin"
    yard = K.yardstick(w, pos, dt, h, B, it)
    print(K.line(case, it, yard, yard))
    assert K.check(case, yard, yard) == []


def test_plants_cover_the_edges():
    for w in K.WIDTHS + (304,):
        pl = K.plants(w, 2)
        cols = {(i, j) for _, i, j in pl}
        assert {(0, 0), (1, 0), (w - 1, w - 1)} <= cols
        cw = K.chunk_width(w)
        if w > cw:
            assert {j for _, j in cols} >= {cw - 1, cw}
        rows_of_col0 = [y for y, i, j in pl if j == 0]
        assert len(set(rows_of_col0)) == len(rows_of_col0)


# lanes per row, chunks -> widths, and per dtype the TRI widths among them (positivity on, switch on)
CLASSES = {
    (16, 1): (8, 16, 128), (16, 2): (136, 256), (16, 3): (264, 272, 304, 360, 368, 384),
    (32, 2): (512,), (32, 3): (520,), (64, 2): (1024,), (64, 3): (1032, 1536),
}


def test_dispatch_classes_and_tri_limits():
    for (gl, nch), ws in CLASSES.items():
        for w in ws:
            assert (K.lanes(w), K.chunks(w)) == (gl, nch), w
    assert set(w for ws in CLASSES.values() for w in ws) == set(K.WIDTHS) | {304}
    # first and last width of every class: a full last chunk, and a last chunk that only the first lane touches
    for gl, nch, lo, hi in ((16, 1, 8, 128), (16, 2, 136, 256), (16, 3, 264, 384), (32, 2, 392, 512), (32, 3, 520, 768), (64, 2, 776, 1024),
                            (64, 3, 1032, 1536)):
        assert (K.lanes(lo), K.chunks(lo)) == (K.lanes(hi), K.chunks(hi)) == (gl, nch)
        assert (K.lanes(hi + 8), K.chunks(hi + 8)) != (gl, nch) or hi == 1536
    tri = lambda dt: [w for w in range(8, 392, 8) if K.uses_tri(w, dt, True)]
    assert tri("float16") == list(range(8, 368, 8))                  # ... 360 | 368
    assert tri("float32") == list(range(8, 272, 8))                  # ... 264 | 272: three chunks with an fp32 triangle at 264 only
    assert not any(K.uses_tri(w, dt, False) for w in K.WIDTHS for dt in K.TDT)
    assert not any(K.uses_tri(w, dt, True) for w in (392, 512, 1536) for dt in K.TDT)
    assert not K.uses_tri(136, "float16", True, switch_on=False)


# ---- the comparator has teeth ------------------------------------------------------------------------------------------------------------
W_T, POS_T, DT_T = 136, True, "float16"


def _run(mutate):
    case, ref, yard = K.build(W_T, POS_T, DT_T), K.reference(W_T, POS_T, DT_T), K.yardstick(W_T, POS_T, DT_T)
    disp, conf, occ, ind = (t.clone() for t in K.oracle_fp32(W_T, POS_T, DT_T))
    out = mutate(case, disp, conf, occ, ind) or (disp, conf, occ, ind)
    return K.check(case, K.compare(case, ref, *out), yard)


def test_comparator_rejects_one_sweep_less():
    assert _run(lambda case, *o: K.oracle_fp32(W_T, POS_T, DT_T, ot_iter=2))


def test_comparator_rejects_an_unmasked_triangle():
    from oracle import s2m2_oracle as O

    def unmasked(case, *o):
        P = O.sinkhorn_prob(case.cv, False)
        d, c, oc, ind = O.regress(P)
        return d[:, 0], c[:, 0], oc[:, 0], ind
    assert _run(unmasked)


def test_comparator_rejects_a_shifted_plant():
    def shift(case, disp, conf, occ, ind):
        y, i, j = case.planted[-1]
        ind[:, y, i] = j + 1
    assert any("planted" in m for m in _run(shift))


def test_comparator_rejects_a_window_without_its_last_tap():
    def short(case, disp, conf, occ, ind):
        from oracle import s2m2_oracle as O
        P = O.sinkhorn_prob(case.cv, case.pos)
        last = torch.gather(torch.nn.functional.pad(P, (0, 2)), 3, (ind + 2)[..., None])[..., 0]
        conf -= last
    assert any(m.startswith("conf") for m in _run(short))


def test_comparator_rejects_nan_and_mass_above_one():
    def nan(case, disp, conf, occ, ind):
        disp[0, 0, 5] = float("nan")
    assert "an output is not finite" in _run(nan)

    def heavy(case, disp, conf, occ, ind):
        occ[0, 1, 7] = 1.0 + 3e-5
    assert any("not in [0, 1 + 1e-5]" in m for m in _run(heavy))
