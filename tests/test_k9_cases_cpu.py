"""The K9 cases of tests/k9_cases.py without the kernel: every form, tile height, stage count and fan-out count is selected by at least one
case according to the host program of tests/test_select_cpu.py; the exact regime's sums stay within 2048 and its reference is representable;
the reference agrees with torch's own fp32 chain; the emulation passes every bound through the comparator the GPU test uses; the ensemble
bound passes every member built from the others; every wrong variant is rejected on every case it applies to; the one-pass variance of the
hot constant is negative before the clamp at every width; CHAIN_RATIO is re-measured; the plain operands pack to what engine.Layer packs.
The tall-tile cases (more than 8000 rows) take part with their exact and analytic bounds; their ensembles are the GPU test's."""
import pytest
import torch
import torch.nn.functional as F

import k9_cases as K

CASES = K.all_cases()
SMALL = [c for c in CASES if c.rows <= 2000]
LIGHT = [c for c in CASES if c.rows <= 2000 or c.kind != "ensemble"]
ENSEMBLE = [c for c in SMALL if c.kind == "ensemble"]


def test_every_form_height_stage_and_fan_count_is_selected():
    sel = {c: K.chosen(c) for c in CASES}
    for c, s in sel.items():
        assert s == c.expected, (c.id, s, c.expected)
    got = {(c.form, c.C, c.dtype, c.bm) for c in CASES}
    want = {("staged", C, K.F16, bm) for C, bm in K.STAGED16} | {("staged", C, K.F32, bm) for C, bm in K.STAGED32}
    want |= {(form, C, K.F16, bm) for form in ("direct", "fan_only") for C, bm in K.DIRECT}
    assert got == want
    for key in want:
        sub = [c for c in CASES if (c.form, c.C, c.dtype, c.bm) == key]
        form, C, dt, bm = key
        if form == "fan_only":
            assert {c.nfan for c in sub} <= {1, 2, 3, 4} and {c.fan_ln for c in sub} == {True, False}, key
        else:
            assert any(c.chain == "attn_tail" and c.regime == r for c in sub for r in ("exact",)) and any(c.chain == "attn_tail" and c.regime == "gauss" for c in sub), key
        if bm == 64:
            T = K.TALL_T[("direct" if form == "fan_only" else form, C)]
            assert {c.rows for c in sub} == {T + 1, T + 101}, key
            assert any(c.rows == T and c.bm == 32 and c.C == C and c.form == form for c in CASES), key
        if any(c.any_ln for c in sub) and dt == K.F16:
            assert any(c.hot for c in sub), key
    assert {c.nstage for c in CASES} == {0, 1, 2, 3} and {c.nfan for c in CASES} == {0, 1, 2, 3, 4}
    assert {c.nfan for c in CASES if c.form == "fan_only"} == {1, 2, 3, 4}
    assert {c.nfan for c in CASES if c.nstage and c.nfan} >= {1, 2, 3, 4}
    assert {c.rows for c in CASES if c.bm == 32 and not c.pool} >= set(K.SHORT_ROWS)
    assert {c.pool for c in CASES if c.pool} == set(K.POOL_GRIDS)
    assert {c.xcd_tiles for c in CASES} >= {0, 1, 2}
    assert any(c.xcd and c.xcd_tiles == 0 and c.form != "fan_only" for c in CASES)          # a hint that is no tile multiple
    four = {("staged", 128, K.F16), ("direct", 256, K.F16), ("direct", 192, K.F16), ("staged", 128, K.F32)}
    for chain in K.CHAINS:
        if chain in ("fan", "pooled", "pass", "attn_tail"):
            continue
        assert {(c.form, c.C, c.dtype) for c in CASES if c.chain == chain} >= four, chain
    for fam in ("staged", "direct", "fan_only"):
        sub = [c for c in CASES if c.form == fam]
        assert {c.xs - c.C for c in sub} == {0, 8, 2 * sub[0].C} or {(c.xs == c.C, c.xs == c.C + 8, c.xs == 3 * c.C) for c in sub} == {(True, False, False), (False, True, False), (False, False, True)}, fam
        if fam != "fan_only":
            assert any(c.rs == c.C + 16 and c.ch.res_stage >= 0 for c in sub) and any(c.os == c.C + 8 for c in sub), fam
            assert any(c.ls == c.C + 24 and c.ln_out for c in sub), fam
        assert any(c.nfan and c.fs == c.nfan * c.C + 8 for c in sub), fam


@pytest.mark.parametrize("C", (128, 192, 256, 384, 512))
def test_hot_constant_has_a_negative_one_pass_variance(C):
    value, var = K.hot_search(C)
    assert value == K.HOT[C] and var < 0
    row = torch.full((1, C), K.HOT[C], dtype=torch.float64)
    _, r0 = K.fold_stats(row, K.F16, K.EPS, clamp=False)
    _, r1 = K.fold_stats(row, K.F16, K.EPS, clamp=True)
    assert bool(torch.isnan(r0).all()) and abs(float(r1) - K.EPS ** -0.5) < 1e-3    # the clamp decides


@pytest.mark.parametrize("case", [c for c in LIGHT if c.regime == "exact"], ids=lambda c: c.id)
def test_exact_claims(case):
    top, pooled_ok = K.exact_sums(case)
    assert top <= 2048 and pooled_ok, (top, pooled_ok)
    K.reference(case)                                                                # asserts ref.to(dtype) == ref


def _torch32(case):
    """the chain by torch's own fp32 layers"""
    inp, ops, ch = K.inputs(case), K.operands(case), case.ch
    if case.pool:
        x = F.avg_pool2d(inp.x.float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).reshape(case.rows, case.C)
    else:
        x = inp.x.float().reshape(case.rows, case.C)
    ln = lambda t, eps: F.layer_norm(t, (case.C,), None, None, eps)                 # noqa: E731
    t, ys = x, []
    for s in range(case.nstage):
        y = F.linear(ln(t, K.EPS) if ch.ln[s] else t, ops.W[s].float(), ops.b[s])
        y = F.gelu(y) if ch.acts[s] == K.GELU else F.relu(y) if ch.acts[s] == K.RELU else y
        if s == ch.res_stage:
            y = y + inp.res.float()
        if ch.carry and s == 2:
            y = y + ys[0]
        ys.append(y)
        t = y
    out = t if case.nstage else None
    lno = F.layer_norm(out, (case.C,), ops.gout, ops.bout, K.LN_OUT_EPS) if case.ln_out else None
    fan = None
    if case.nfan:
        fan = F.linear(ln(t, K.EPS) if case.fan_ln else t, ops.fanW.float().reshape(-1, case.C), ops.fanb)
    return out, lno, fan


@pytest.mark.parametrize("case", SMALL[::3], ids=lambda c: c.id)
def test_reference_agrees_with_torch_fp32(case):
    ref = K.reference(case)
    for got, want in zip(_torch32(case), (ref.out, ref.ln, ref.fan)):
        assert (got is None) == (want is None)
        if want is not None:
            tol = 2e-3 * max(1.0, float(want.abs().max())) * (10.0 if case.regime == "pass" or case.any_ln else 1.0)
            assert float((got.double() - want).abs().max()) <= tol, case.id


@pytest.mark.parametrize("case", LIGHT, ids=lambda c: c.id)
def test_emulation_passes(case):
    j = K.judge(case)
    for m in j.members:
        for what, res in K.verdict(case, m):
            assert res.ratio <= 1, K.line(case, what, res)


@pytest.mark.parametrize("case", ENSEMBLE, ids=lambda c: c.id)
def test_leave_one_out(case):
    """every member of the ensemble passes the bound built from the other eight: the factor 2 is not too tight"""
    j = K.judge(case)
    for i, m in enumerate(j.members):
        others = [o for k, o in enumerate(j.members) if k != i]
        for w in range(3):
            if j.ref[w] is not None:
                res = K.K13.compare(m[w], j.ref[w], K.K13.token_bound(j.ref[w], [o[w] for o in others]))
                assert res.ratio <= 1, (i, K.line(case, K.WHAT[w], res))


def _rejects(case, variant):
    return [f"{what} ratio {res.ratio:.3g} at {res.where}" for what, res in K.verdict(case, K.emulate(case, variant)) if not res.ratio <= 1]


@pytest.mark.parametrize("variant", K.VARIANTS)
def test_every_wrong_variant_is_rejected_wherever_it_applies(variant):
    tried, passed = 0, []
    for case in SMALL:
        if not K.applies(variant, case) or K.exempt(variant, case):
            continue
        tried += 1
        if not _rejects(case, variant):
            passed.append(case.id)
    assert tried > 0, variant
    assert not passed, f"{variant}: passes on {len(passed)} of {tried} cases it applies to: {passed}"


def test_variants_reach_the_form_families():
    """the variants of the weight stream and of the fold are rejected on a staged, a direct and a fan-out-only case, in both dtypes where they exist"""
    for variant in ("k16_halves_swapped", "frag_tile_stride", "ln_eps_1e-6", "ln_no_clamp"):
        fams = {(c.form, c.dtype) for c in SMALL if K.applies(variant, c) and not K.exempt(variant, c)}
        want = {("staged", K.F16), ("direct", K.F16), ("fan_only", K.F16)} | ({("staged", K.F32)} if variant != "ln_no_clamp" else set())
        assert fams >= want, (variant, fams)


def test_what_no_comparison_shows():
    """NOT_SHOWN: ln_out from the unrounded sum passes the comparator (it is closer to the reference), so it is no member of VARIANTS"""
    assert set(K.NOT_SHOWN) == {"ln_out_from_unrounded", "last_tile_stores_all_rows"} and not set(K.NOT_SHOWN) & set(K.VARIANTS)
    for case in [c for c in SMALL if c.chain in ("norm_only", "pass") and c.regime != "exact"][:6]:
        for what, res in K.verdict(case, K.emulate_ln_out_from_unrounded(case)):
            assert res.ratio <= 1, K.line(case, what, res)


def test_guard_logic_on_a_fake_output():
    """last_tile_stores_all_rows: one row too many lands in the NaN row behind the slice, which outside_is_nan() sees"""
    rows, C, stride = 33, 128, 136
    pad = K.pad_of(stride, C)
    whole = torch.full((rows + 2, stride), float("nan"))
    mask = torch.zeros_like(whole, dtype=torch.bool)
    mask[1:-1, pad:pad + C] = True
    whole[1:-1, pad:pad + C] = 1.0
    assert K.outside_is_nan(whole, mask)
    for r, c in ((rows + 1, pad), (0, pad + C - 1), (5, pad + C)):                  # the row behind, the row in front, a channel past the slice
        w = whole.clone()
        w[r, c] = 0.0
        assert not K.outside_is_nan(w, mask)


def test_chain_ratio_of_the_forward():
    """the figure CHAIN_RATIO quotes: the largest |mean| / std of a row entering a pre-LayerNorm or DispInit's LayerNorm of the S forward"""
    from oracle import s2m2_oracle as O
    from s2m2_amd.weights import seeded_state_dict, synthetic_pair
    seen, inner_ln, inner_corr = [], O._ln, O.ln_corr

    def rec(t):
        t = t.double()
        seen.append(float((t.mean(-1).abs() / t.std(-1, unbiased=False)).max()))

    def ln(x):
        rec(x)
        return inner_ln(x)

    def corr(feat, gamma, beta):
        rec(feat.permute(0, 2, 3, 1))
        return inner_corr(feat, gamma, beta)
    O._ln, O.ln_corr = ln, corr
    try:
        l, r = synthetic_pair(128, 192, 1, 16, 3)
        O.forward(seeded_state_dict(128, 1, 1, 0), l, r, True, 1, False, {})
    finally:
        O._ln, O.ln_corr = inner_ln, inner_corr
    assert len(seen) >= 20
    assert max(seen) <= K.CHAIN_RATIO, max(seen)
    assert max(K.OFFS) / min(K.SCALES) >= 2 * K.CHAIN_RATIO
    x = K.inputs(next(c for c in SMALL if c.regime == "gauss" and c.rows == 97 and not c.pool)).x.double()
    ratio = x.mean(-1).abs() / x.std(-1, unbiased=False).clamp(min=1e-30)
    assert float(ratio[x.std(-1) > 0].max()) > 12.0


def test_operands_equal_the_engines_packing():
    """pack_layer() is engine.Layer.stage() / .fan() on one layer of seeded_state_dict"""
    from s2m2_amd import engine, pack
    from s2m2_amd.weights import seeded_state_dict
    sd = seeded_state_dict(128, 1, 1, 0)
    name = "transformer.uformer_list.0.enc_attn0.ffn.ffn.0"
    w, b = sd[name + ".weight"], sd[name + ".bias"]
    for dtype, frag in ((K.F16, True), (K.F16, False), (K.F32, False)):
        layer = engine.Layer(pack.pack_conv(w, K.TDT[dtype]), pack.pack_bias(b, w.shape[0]), 1, 1, w.shape[0])
        wp, wsum = K.pack_layer(w.to(K.TDT[dtype]), dtype, frag)
        sw, sb, act, sws = layer.stage(K.GELU, frag=frag, ln=True)
        assert torch.equal(sw, wp) and torch.equal(sws, wsum) and torch.equal(sb, pack.pack_bias(b, w.shape[0])) and act == K.GELU
        if frag:
            fw, fb, fws = layer.fan(ln=True)
            assert torch.equal(fw, wp) and torch.equal(fws, wsum)
