"""The K13 cases of tests/k13_cases.py without the kernel: the widths reach every wave count, both instantiations, one and two key chunks
and every class of the entry phase's counted wait, computed as csrc/rowattn.hip computes them; the magnets dominate; the pre-activations
stay where the GELU figure holds; the emulation passes every case through the comparator the GPU test uses; the per-token bound of the full
regime passes every member of its own ensemble built from the others; every wrong variant is rejected, and the failure text of a variant
that is not names the cases that were tried; the plain operands pack to what the engine packs."""
import pytest
import torch

import k13_cases as K

CASES = K.all_cases()
FULL = [c for c in CASES if c.regime == "full"]
ROUTE = [c for c in CASES if c.regime in K.ROUTED]
TAIL = [c for c in CASES if c.regime == "tail"]


def test_widths_reach_every_wave_count_chunk_and_wait_class():
    by_w = {}
    for c in CASES:
        by_w.setdefault(c.w, []).append(c)
    assert set(K.WIDTHS) <= set(by_w)
    assert {c.nwv for c in CASES} == set(range(1, 11))
    assert {c.threads for c in CASES} == {320, 640}
    one = lambda w: by_w[w][0]                                                      # noqa: E731
    assert one(160).threads == 320 and one(160).nchunk == 1 and one(161).threads == 640 and one(161).nchunk == 2
    # the one-key second chunk: a single tile (two projection items dealt to six waves) that holds key 160 alone
    c = one(161)
    assert c.ntile - 5 == 1 and c.w - 160 == 1 and c.nwv == 6
    assert {c.nchunk for c in CASES} == {1, 2}
    assert {c.w % 32 for c in CASES} >= {0, 1, 31}                                  # full, one-token and all-but-one last tiles
    # the entry phase's counted wait: vmcnt(0) at up to four waves, per-wave different counts wherever nwv does not divide 32
    for nwv in range(1, 11):
        c = next(c for c in CASES if c.nwv == nwv)
        waits = {c.entry_wait(wv) for wv in range(nwv)}
        assert all(c.nkv(wv) == 2 * len(range(wv, 32, nwv)) for wv in range(nwv))
        if nwv <= 4:
            assert waits == {0}, (nwv, waits)
        elif 32 % nwv:
            assert len(waits) == 2 and 0 not in waits, (nwv, waits)
        else:
            assert len(waits) == 1 and 0 not in waits, (nwv, waits)                  # nwv = 8
    for w, cs in by_w.items():
        if w in K.WIDTHS:
            assert {(c.heads, c.cross) for c in cs} >= {(1, True), (1, False), (2, True), (2, False)}, w
            assert {c.regime for c in cs} >= {"full", "route"}, w
    for th in (320, 640):
        sub = [c for c in CASES if c.threads == th]
        assert {c.xs for c in sub} == set(K.X_STRIDES) and {c.os for c in sub} == set(K.OUT_STRIDES), th
        assert {c.ln_out for c in sub} == {True, False} and all(c.ls == K.LN_STRIDE for c in sub)
        assert {(c.regime, c.heads) for c in sub} == {(r, hd) for r in ("full", "route") + K.PROBES for hd in (1, 2)}, th
    main = CASES[:4 * len(K.WIDTHS)]
    assert sum(c.ln_out for c in main) * 2 == len(main)
    assert {c.nimg for c in CASES if not c.cross} >= {1, 3} and {c.nimg for c in CASES if c.cross} == {2, 4, 6}
    assert {c.h for c in main} == {1, 2, 3}
    assert all(c.rows <= 96 for c in CASES)
    assert any(c.hot for c in FULL)


def test_xcd_cases_permute_rows():
    xc = [c for c in CASES if c.h % 8 == 0]
    assert {(c.h, c.nimg, c.xcd) for c in xc} == {(h, n, x) for h in (8, 16) for n in (2, 4, 6) for x in (0, 1)}
    assert all(c.regime == "route" for c in xc)
    assert {c.heads for c in xc if c.xcd and c.h > 8} == {1, 2}                      # a permuted launch of either head count
    assert all(len({(c.w, c.heads, c.cross) for c in xc if (c.h, c.nimg) == key}) == 1 for key in {(c.h, c.nimg) for c in xc})
    for c in xc:
        rows = [K.block_row(c, b) for b in range(c.rows)]
        assert sorted(rows) == list(range(c.rows))
        assert (rows != list(range(c.rows))) == bool(c.xcd and c.h > 8)             # (h = 8: one line per XCD, the map is the identity)
        assert [K.block_row(c, b, exchanged=True) for b in range(c.rows)] != rows or not c.xcd
        if c.xcd:
            # the rows of one line in all images are neighbours in dispatch order on one XCD (blocks are dealt round robin to eight)
            assert all(K.block_row(c, b) % c.h == K.block_row(c, b - 8) % c.h for b in range(8, 8 * c.nimg))


@pytest.mark.parametrize("case", ROUTE, ids=lambda c: c.id)
def test_route_magnets_dominate(case):
    t = K.logits64(case)                                                            # (rows, heads, w, w), log2 domain
    pi = K.inputs(case).pi
    top = torch.gather(t, 3, pi[..., None])
    rest = t.scatter(3, pi[..., None], -float("inf")).amax(-1, keepdim=True)
    if case.w > 1:
        assert float((top - rest).min()) > 40.0, float((top - rest).min())
    # the running maximum rises in the last tile visited for at least a quarter of the queries of every head
    last0 = 32 * (case.ntile - 1)
    assert float((pi >= last0).double().mean(-1).min()) >= 0.25
    keys = set(pi.flatten().tolist())
    assert set(K.route_targets(case)) <= keys and {0, case.w - 1} <= keys
    if case.w > 160:
        assert {159, 160} <= keys


@pytest.mark.parametrize("case", FULL, ids=lambda c: c.id)
def test_full_tokens_are_what_the_docstring_says(case):
    x = K.inputs(case).x.double()
    m, s = x.mean(-1), x.std(-1, unbiased=False)
    assert float(s[0, case.w // 2]) == 0.0 and float(m[0, case.w // 2]) == 1.5
    ratio = (m.abs() / s.clamp(min=1e-30))[s > 0]
    assert float(ratio.max()) >= 2 * K.TOKEN_RATIO and float(ratio.max()) > 12.0
    # neighbours differ in offset and in scale
    body = slice(0, min(case.w, 3))
    assert float((m[1 % case.rows, body][1:] - m[1 % case.rows, body][:-1]).abs().min()) > 0.5 or case.w < 3
    # key w - 1 leads the logits of the queries aimed at it
    t = K.logits64(case)
    qi = torch.arange(3, case.w - 1, 10)
    if qi.numel():
        lead = t[:, :, qi].argmax(-1) == case.w - 1
        assert float(lead.double().mean()) > 0.9, float(lead.double().mean())
        assert qi.numel() * 10 >= case.w - 12
    if case.hot:
        hot = x[case.rows - 1, 1:2]
        _, r0 = K.ln_stats(hot, K.EPS, clamp=False)
        _, r1 = K.ln_stats(hot, K.EPS, clamp=True)
        assert bool(torch.isnan(r0).all()) and abs(float(r1) - K.EPS ** -0.5) < 1e-3    # the clamp decides


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_intermediates_stay_in_range(case):
    ref = K.reference(case)
    assert bool(torch.isfinite(ref.out).all()) and float(ref.out.abs().max()) < 200.0
    assert ref.qkv_max < 256.0                                                       # q . k of 128 channels stays far inside fp32, q, k, v inside fp16
    assert float(ref.pre.abs().max()) <= 8.0, float(ref.pre.abs().max())            # where the fast GELU's figures hold (csrc/epilogue.h)
    lg = K.logits64(case)
    assert float((lg.amax(-1, keepdim=True) - lg).max()) < 1000.0                    # exp2 flushes to zero long before: no overflow, no NaN
    out, ln = K.emulate(case)
    assert bool(torch.isfinite(out).all()) and (ln is None or bool(torch.isfinite(ln).all()))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_emulation_passes(case):
    j = K.judge(case)
    for out, ln in j.members:
        for what, res in K.verdict(case, out, ln):
            assert res.ratio <= 1, K.line(case, what, res)


@pytest.mark.parametrize("case", FULL, ids=lambda c: c.id)
def test_leave_one_out(case):
    """every member of the ensemble passes the bound built from the other eight: the factor 2 is not too tight"""
    j = K.judge(case)
    for i, (out, ln) in enumerate(j.members):
        others = [m for k, m in enumerate(j.members) if k != i]
        res = K.compare(out, j.out, K.token_bound(j.out, [m[0] for m in others]))
        assert res.ratio <= 1, (i, K.line(case, "out", res))
        if case.ln_out:
            res = K.compare(ln, j.ln, K.token_bound(j.ln, [m[1] for m in others]))
            assert res.ratio <= 1, (i, K.line(case, "ln", res))


def _rejects(case, variant):
    out, ln = K.emulate(case, variant)
    return [f"{what} ratio {res.ratio:.3g} at {res.where}" for what, res in K.verdict(case, out, ln) if not res.ratio <= 1]


@pytest.mark.parametrize("variant", K.VARIANTS)
def test_every_wrong_variant_is_rejected(variant):
    tried = []
    for case in CASES:
        if not K.applies(variant, case) or K.exempt(variant, case):
            continue
        why = _rejects(case, variant)
        if why:
            print(f"{variant}: rejected on {case.id}: {'; '.join(why)}")
            return
        tried.append(case.id)
    pytest.fail(f"{variant}: passes on every case it applies to: {tried}")


def test_variants_are_rejected_in_both_instantiations_where_they_apply():
    """the variants of the tile walk are rejected on a 320-thread and on a 640-thread case"""
    for variant in ("mask_off_by_one", "padding_unmasked", "ragged_last_from_neighbour", "vstat_wrong_token", "no_rescale_in_tile"):
        for th in (320, 640):
            hit = None
            for case in CASES:
                if case.threads == th and K.applies(variant, case) and not K.exempt(variant, case) and _rejects(case, variant):
                    hit = case
                    break
            assert hit is not None, (variant, th)


def test_exemptions_hold():
    """an exempt case really is blind to its variant: otherwise the exemption would hide a rejection"""
    case = next(c for c in CASES if c.cross and c.nimg == 2 and c.regime == "full")
    assert K.exempt("cross_roll_one", case)
    a, b = K.emulate(case, "cross_roll_one"), K.emulate(case)
    assert torch.equal(a[0], b[0])
    for regime in K.ROUTED:                                                          # the magnet's lead does not need the q bias
        case = next(c for c in CASES if c.regime == regime and c.ln_out)
        assert K.exempt("q_bias_dropped", case)
        a, b = K.emulate(case, "q_bias_dropped"), K.emulate(case)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for regime in ("full", "route", "attn", "ffn", "tail"):                          # ln_out from the unrounded sum, one pass: inside the bound
        case = next(c for c in CASES if c.regime == regime and c.ln_out)
        assert K.exempt("ln_out_onepass_unrounded", case)
        assert not _rejects(case, "ln_out_onepass_unrounded"), case.id
    # every other pair (variant, case) that applies is a candidate
    assert all(K.exempt(v, c) is None for v in K.VARIANTS for c in CASES
               if v not in ("cross_roll_one", "q_bias_dropped", "ln_out_onepass_unrounded") and K.applies(v, c))


@pytest.mark.parametrize("case", TAIL, ids=lambda c: c.id)
def test_tail_probe_owes_z1_exactly_and_rejects_a_wrong_proj_stage(case):
    ref = K.reference(case)
    assert torch.equal(ref.z1.half().double(), ref.z1) and float(ref.z1.abs().max()) <= 4.0
    assert float((ref.z1 * 16 - (ref.z1 * 16).round()).abs().max()) == 0.0
    ops = K.ops_of(case)
    assert bool((ops.b[3] != 0).all()) and bool((ops.W[2] == 0).all())
    for variant in ("proj_bias_dropped", "residual_from_o", "residual2_from_x", "cols_unrelabelled"):
        assert _rejects(case, variant), (variant, case.id)


def test_token_ratio_of_the_forward():
    """the figure TOKEN_RATIO quotes: the largest |mean| / std of a token entering or leaving a 1-D attention block of the S forward"""
    from oracle import s2m2_oracle as O
    from s2m2_amd.weights import seeded_state_dict, synthetic_pair
    seen, inner = [], O.basic_attn_block

    def wrapped(sd, p, z, nh):
        out = inner(sd, p, z, nh)
        for t in (z, out):
            if t.shape[1] == 128:                                                    # the 1/4 and 1/8 levels: the widths K13 takes
                seen.append(float((t.mean(1).abs() / t.std(1, unbiased=False)).max()))
        return out
    O.basic_attn_block = wrapped
    try:
        l, r = synthetic_pair(128, 192, 1, 16, 3)
        O.forward(seeded_state_dict(128, 1, 1, 0), l, r, True, 1, False, {})
    finally:
        O.basic_attn_block = inner
    assert len(seen) >= 8
    assert max(seen) <= K.TOKEN_RATIO, max(seen)
    assert max(K.OFFS) / min(K.SCALES) >= 2 * K.TOKEN_RATIO


def test_operands_equal_the_engines_packing(monkeypatch):
    """make_ops() with no pre-LN affine (the reference model has none) packs to exactly what Engine.row_step hands the kernel for a
    BasicAttnBlock of seeded_state_dict: weights, the four row sums, the biases the model has, zero rows for those it has not."""
    import s2m2_amd.engine as engine_mod
    from fake_hip import make as fake_hip
    from s2m2_amd.model import S2M2
    from s2m2_amd.weights import seeded_state_dict
    fake, got = fake_hip(), {}

    def row_attn(z, nh, cross, wts, vec, ln_eps=1e-5, ln_out_eps=None, xcd_hint=True):
        got[bool(cross)] = (wts, vec)
        return z if ln_out_eps is None else (z, z)
    fake.row_attn = row_attn
    monkeypatch.setattr(engine_mod, "hip", fake)
    sd = seeded_state_dict(128, 1, 1, 0)
    m = S2M2(128, 1, 1, use_positivity=True, refine_iter=1)
    m.load_state_dict(sd, strict=True)
    eng = engine_mod.Engine(m, torch.float16)
    p = "transformer.uformer_list.0.enc_attn0"
    z = torch.zeros(2, 1, 8, 128, dtype=torch.float16)
    eng.row_step(p + ".cross_attn", p + ".ffn_c", z, 1, True)
    gam, bet = torch.rand(128) + 0.5, torch.randn(128)
    eng.row_step(p + ".self_attn", p + ".ffn", z, 1, False, ln_out=(gam, bet, 1e-5))
    for cross, pa, pf, aff in ((True, p + ".cross_attn", p + ".ffn_c", None), (False, p + ".self_attn", p + ".ffn", (gam, bet))):
        names = [pa + ".attn.q", pa + ".attn.k", pa + ".attn.v", pa + ".attn.proj", pf + ".ffn.0", pf + ".ffn.2"]
        ops = K.make_ops([(sd[n + ".weight"], sd.get(n + ".bias")) for n in names], None, None, aff)
        assert ops.b[0] is None and ops.b[1] is None and ops.b[3] is None and ops.b[2] is not None
        wts, vec = K.packed(ops)
        assert torch.equal(wts, got[cross][0]) and torch.equal(vec, got[cross][1])
        assert bool((vec[[0, 2, 6]] == 0).all()) and bool((vec[[4, 7, 9]] != 0).any())


def test_fold_is_the_affine_pre_layernorm():
    """fold(): W (n gamma + beta) + b == W' n + b' up to the fp16 rounding of W'"""
    g = torch.Generator().manual_seed(5)
    w, b = torch.randn(128, 128, generator=g) / 128 ** 0.5, torch.randn(128, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(128, generator=g), 0.2 * torch.randn(128, generator=g)
    n = torch.randn(7, 128, generator=g).double()
    wf, bf = K.fold(w, b, gamma, beta)
    want = (n * gamma.double() + beta.double()) @ w.double().T + b.double()
    got = n @ wf.double().T + bf.double()
    assert float((want - got).abs().max()) < 128 * 2.0 ** -11 * 0.3 * 4
    w0, b0 = K.fold(w, None)
    assert b0 is None and torch.equal(w0, w.half())
