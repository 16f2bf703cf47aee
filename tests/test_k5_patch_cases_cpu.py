"""The construction of the K5 patch-kernel tests (tests/k5_patch_cases.py) without the kernels: the float64 reference agrees with torch's own
fp32 F.conv2d inside the bound the GPU test uses, the `exact` cases are representable in both I/O dtypes, the comparator takes the rounded
reference and nothing one element away from it, the explicit patch gather is the layer for every patch form, each of the twelve wrong patch
loaders is rejected wherever it differs by construction, the cases cover what the module's docstring claims, and the SIGMOID / TANH figures of
k5_cases.act_abs() hold against a float32 restatement of csrc/epilogue.h's two formulas with exp2 and the reciprocal moved by an ulp."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import k5_cases as K
import k5_patch_cases as P

DTYPES = ("float32", "float16")
IDS = ("fp32", "fp16")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", P.NAMES)
def test_reference_vs_torch_fp32(name, dtype):
    """torch's fp32 convolution of the same operands, pushed through the comparator the kernels face"""
    c, ref = P.build(name, dtype), P.reference(name, dtype)
    L = c.layer
    x = torch.cat(c.xs, -1).permute(0, 3, 1, 2)
    pre = F.conv2d(x, c.w, c.b, padding=(L.KH // 2, L.KW // 2)).permute(0, 2, 3, 1)
    assert pre.dtype == torch.float32 and tuple(pre.shape) == (c.N, c.H, c.W, L.Cout)
    res = K.compare(c, ref, K.finish(c, pre.double()) + 0.0)
    print(K.line(c, "F.conv2d (fp32)", res))
    assert not res.bad, "; ".join(res.bad)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_cases_are_representable(dtype):
    names = [n for n in P.NAMES if P.SPECS[n].regime == "exact"]
    assert len(names) >= 35
    for name in names:
        c, ref = P.build(name, dtype), P.reference(name, dtype)
        assert ref.bound is None and c.spec.act in (K.ACT_NONE, K.ACT_RELU) and c.spec.epi == K.EPI_NONE
        S = K._conv64([x.abs() for x in c.xs], c.w.abs(), c.layer) + c.b.abs().double()
        assert float(S.max()) <= K.EXACT_MAX, name                       # every partial sum, in any order, is an integer of at most 2048
        for t in c.xs + (c.w, c.b):
            assert torch.equal(t, t.round()) and torch.equal(t.to(K.TDT[dtype]).float(), t)
        assert torch.equal(ref.out, ref.out.round()) and torch.equal(ref.out.to(K.TDT[dtype]).double(), ref.out), name
        assert all(bool((x != 0).all()) for x in c.xs)                   # a pixel read where the zero block belongs always changes a product
        assert float(ref.out.abs().max()) > 8, name


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", P.NAMES)
def test_comparator_accepts_the_rounded_reference(name, dtype):
    c, ref = P.build(name, dtype), P.reference(name, dtype)
    res = K.compare(c, ref, ref.out.to(K.TDT[dtype]))
    assert not res.bad and res.ratio <= (0.0 if ref.bound is None else 1.0), res


@pytest.mark.parametrize("name", ["3x3_128-3x9x70-exact", "1x3_zr-3x9x70-gauss-sigmoid-mul", "3x1_128+128-1x5x41-gauss-tanh-gru"])
def test_comparator_judges_every_element(name):
    for dtype in DTYPES:
        c, ref = P.build(name, dtype), P.reference(name, dtype)
        good = ref.out.to(K.TDT[dtype])
        for at in ((c.N - 1, c.H - 1, c.W // 2, 5), (0, 0, c.W - 1, c.layer.Cout - 1)):       # (below and above epi_cout0)
            one = good.clone().double()
            one[at] += 1.0 if ref.bound is None else 2.5 * float(ref.bound[at])
            res = K.compare(c, ref, one)
            assert len(res.bad) == 1 and res.where == at and res.bad[0].startswith("1 elements"), res
        nan = good.clone()
        nan[0, 0, 0, 0] = float("nan")
        assert K.compare(c, ref, nan).where == (0, 0, 0, 0) and K.compare(c, ref, nan).bad
        assert K.compare(c, ref, good[:, :-1]).bad and K.compare(c, ref, good[..., :-8]).bad
    if P.SPECS[name].regime == "gauss":                                  # an fp16 result passes its own bound, not the fp32 one
        assert K.compare(P.build(name, "float32"), P.reference(name, "float32"), P.reference(name, "float32").out.half()).bad


def _same(ref, got):
    if ref.bound is None:
        return torch.equal(got, ref.out)
    return float((got - ref.out).abs().max()) <= 1e-12 * max(1.0, float(ref.out.abs().max()))


@pytest.mark.parametrize("name", P.NAMES)
def test_the_gather_is_the_layer(name):
    """wrong(case, None, PH, PW, CH, BN) -- patch origin, halo pixel, zero block, chunk of pieces, (chunk, tap) weights -- is F.conv2d, for every
    patch form the case is launched on (fp16: the halo tile's and the fragment stream's; fp32: the halo tile's 32-channel chunks)"""
    seen = 0
    for dtype in DTYPES:
        c, ref = P.build(name, dtype), P.reference(name, dtype)
        for PH, PW, CH, BN in dict.fromkeys((f[0], f[1], f[2], 0) for f in P.forms(c)):       # (BN changes nothing in the layer itself)
            assert _same(ref, P.wrong(c, None, PH, PW, CH)), (name, dtype, PH, PW, CH)
            seen += 1
    assert seen >= 1


@pytest.mark.parametrize("variant", P.VARIANTS)
def test_wrong_variants_are_rejected(variant):
    """on every case and patch form where the variant differs by construction it is rejected; where it does not, it is the layer and passes.
    If a differing one passes, the inputs are too tame."""
    exact, total = 0, 0
    for name in P.NAMES:
        for dtype in DTYPES:
            c, ref = P.build(name, dtype), P.reference(name, dtype)
            done = {}
            for form in P.forms(c):
                key = tuple(form[i] for i in P.DEPENDS.get(variant, ()))
                d = P.differs(c, variant, *form)
                if key in done:
                    assert done[key] == d
                    continue
                done[key] = d
                res = K.compare(c, ref, P.wrong(c, variant, *form))
                if d:
                    total += 1
                    exact += ref.bound is None
                    assert res.bad, f"the wrong variant {variant} passes {name} {dtype} {form}"
                else:
                    assert not res.bad, f"{variant} is said not to differ on {name} {dtype} {form}: {res.bad}"
    print(f"{variant}: rejected on {total} (case, dtype, form) triples, {exact} of them bit for bit")
    assert total >= 2 and (exact >= 1 or variant == "epi_cout0_ignored")  # (an epilogue has no exact regime)


def test_cases_cover_what_they_claim():
    S = P.SPECS
    by = lambda layer, regime=None: {S[n].shape for n in P.NAMES if S[n].layer == layer and regime in (None, S[n].regime)}
    assert by("3x3_128", "exact") >= set(P.SHAPES) and len(P.SHAPES) == 13
    assert {S[n].layer for n in P.NAMES} == set(P.LAYERS) and len(P.LAYERS) == 13
    for layer in P.LAYERS:
        assert P.RAGGED in by(layer, "exact") and P.OVER in by(layer) and by(layer) & set(P.ONE_PATCH), layer
    assert P.frag_layers() == ("3x3_128", "3x3_256", "3x1_128+128", "1x3_128+128", "1x3_zr", "3x3_96+64+32_384", "3x3_128+128+64+64", "3x3_192",
                               "1x3_192+192", "3x3_96+96_576")
    assert {l: P.frag_chunk(P.LAYERS[l]) for l in ("3x3_192", "1x3_192+192", "3x3_96+96_576", "3x3_96+64+32_384", "3x3_256")} == \
        {"3x3_192": 192, "1x3_192+192": 192, "3x3_96+96_576": 192, "3x3_96+64+32_384": 128, "3x3_256": 128}
    gauss = [S[n] for n in P.NAMES if S[n].regime == "gauss"]
    assert {s.act for s in gauss} == {0, 1, 2, 3, 4} and {s.epi for s in gauss} == {0, 1, 2, 3, 4} and {s.scale for s in gauss} == {1.0, 0.5}
    assert all(s.act in (K.ACT_NONE, K.ACT_RELU) for s in S.values() if s.regime == "exact")
    for epi in (K.EPI_GRU, K.EPI_GATEMIX):                               # where the forward uses them
        assert {s.layer for s in gauss if s.epi == epi} >= {"3x1_128+128", "1x3_128+128"}
        assert all(P.LAYERS[s.layer].KH * P.LAYERS[s.layer].KW == 3 for s in gauss if s.epi == epi)
    zr = [s for s in gauss if s.epi_cout0]
    assert zr and all(s.layer == "1x3_zr" and s.epi_cout0 == 128 and s.halo == () for s in zr)
    assert any(s.act == K.ACT_SIGMOID and s.epi == K.EPI_MUL for s in zr)
    # every halo tile id and every fragment-stream form, on 128- and on 192-cout blocks, is met by an exact and by a gauss case
    for regime in ("exact", "gauss"):
        ss = [s for s in S.values() if s.regime == regime]
        assert set().union(*(s.halo for s in ss)) == set(P.HALO)
        for ck in (128, 192):
            assert set().union(*(s.frag for s in ss if s.frag and P.frag_chunk(P.LAYERS[s.layer]) == ck)) == set(P.FRAG), (regime, ck)
    for s in S.values():                                                 # the refused combinations are left out by rule, nothing else is
        assert set(s.halo) in (set(), set(P.HALO))
        want = () if s.layer not in P.frag_layers() else tuple(t for t in P.FRAG if (s.epi, t) not in P.REFUSED)
        assert s.frag == want
    # every wrong loader differs on at least two cases (a variant taken out of VARIANTS fails here)
    counted = _cases_differing()
    assert set(counted) == set(P.VARIANTS) == {"image_wrap", "row_wrap", "pad_less", "stride_of_src0", "seam_zero", "chunk_tail_reads_on",
                                               "src_boundary_at_chunk", "raster_32", "chunk_tap_swapped", "cout_block_stride",
                                               "epi_cout0_ignored", "partial_patch_stored"}
    assert all(v >= 2 for v in counted.values()), counted
    # the poison is where the docstring says
    two = P.build("3x3_8+128_136-3x9x70-exact-relu")
    big = K.wide(two, 1)
    assert K.wide(two, 0).shape[-1] != big.shape[-1] and big.shape[0] == two.N + 2
    assert bool(torch.isnan(big[0]).all()) and bool(torch.isnan(big[-1]).all()) and bool(torch.isnan(big[..., :K.PAD]).all())
    assert bool(torch.isnan(big[..., -K.PAD:]).all()) and torch.equal(big[1:-1, :, :, K.PAD:-K.PAD], two.xs[1])


def test_every_launch_runs_the_kernel_it_names():
    """every launch of every case through csrc/conv_select.h on the host: a forced tile gives exactly the form it names (never another one in
    its place), the heuristic stays inside the family, and what is SELECTED -- not what is requested -- covers every halo instantiation in both
    dtypes and every fragment-stream form on both block widths, without an operand and with one, in the exact and in the gauss regime"""
    seen = set()
    for name in P.NAMES:
        for dtype in DTYPES:
            c = P.build(name, dtype)
            for l in P.launches(c):
                got, want = P.chosen(c, l), P.forced(c, l)
                assert not got.startswith("E:"), (name, dtype, l.what, got)
                assert got.split()[0] == ("frag" if l.korder == 2 else "halo"), (name, dtype, l.what, got)
                if want is not None:
                    assert got == want, f"{name} {dtype} {l.what}: asked for {want}, conv_select chose {got}"
                seen.add((c.spec.regime, dtype, got))
    halo = {"halo 128 4 2 1", "halo 64 4 2 1", "halo 128 8 2 1", "halo 64 8 4 1", "halo 64 8 4 4", "halo 64 4 2 4", "halo 128 8 2 2"}
    for regime in ("exact", "gauss"):
        for dtype in DTYPES:
            assert {g for r, d, g in seen if (r, d) == (regime, dtype) and g.startswith("halo")} == halo, (regime, dtype)
        frag = {g for r, d, g in seen if r == regime and g.startswith("frag")}
        assert frag >= {f"frag {ck} {ck} {ph} {pw} 0" for ck in (128, 192) for ph, pw in ((2, 32), (4, 32), (4, 40))}, (regime, sorted(frag))
    frag = {g for r, d, g in seen if r == "gauss" and g.startswith("frag")}
    assert frag >= {f"frag {ck} {ck} {ph} {pw} 1" for ck in (128, 192) for ph, pw in ((2, 32), (4, 32), (4, 40))}, sorted(frag)
    assert frag >= {"frag 128 128 2 32 2", "frag 192 192 2 32 2"}
    one = P.build("3x3_128-1x4x40-exact-relu")                          # the grid that is exactly one 4x40 patch runs as one
    assert P.chosen(one, [l for l in P.launches(one) if l.tile == 40][0]) == "frag 128 128 4 40 0"


def _cases_differing():
    """variant -> the number of cases it differs on (some dtype, some form)"""
    out = {}
    for v in P.VARIANTS:
        out[v] = sum(any(P.differs(P.build(n, dt), v, *f) for dt in DTYPES for f in P.forms(P.build(n, dt))) for n in P.NAMES)
    return out


# ---- the SIGMOID / TANH figures of k5_cases.act_abs() ------------------------------------------------------------------------------------
L2E = np.float32(1.44269504088896340736)


def _moved(v, k):
    """float32 array moved by k ulp"""
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return v


def _device(x, act, ke, kr):
    """csrc/epilogue.h in numpy float32, every operation rounded once; exp2 and the reciprocal correctly rounded, then moved by ke / kr ulp"""
    t = (-x if act == K.ACT_SIGMOID else np.float32(2.0) * x) * L2E
    assert t.dtype == np.float32
    e = _moved(np.exp2(t.astype(np.float64)).astype(np.float32), ke)
    s = np.float32(1.0) + e
    r = _moved((1.0 / s.astype(np.float64)).astype(np.float32), kr)
    return r if act == K.ACT_SIGMOID else np.float32(1.0) - np.float32(2.0) * r


@pytest.mark.parametrize("act", [K.ACT_SIGMOID, K.ACT_TANH], ids=["sigmoid", "tanh"])
def test_sigmoid_and_tanh_figures_hold_for_the_headers_formulas(act):
    x = np.linspace(-K.EXP_RANGE, K.EXP_RANGE, 400_001).astype(np.float32)
    x64 = torch.from_numpy(x.astype(np.float64))
    true = K.activate(x64, act).numpy()
    fig = K.act_abs(x64, act).numpy()
    worst = np.zeros_like(true)
    for ke, kr in itertools.product((-1, 0, 1), repeat=2):
        got = _device(x, act, ke, kr)
        assert got.dtype == np.float32
        worst = np.maximum(worst, np.abs(got.astype(np.float64) - true))
    print(f"act {act}: worst error / figure {float((worst / fig).max()):.3f}, figure <= {float(fig.max() / K.U24):.2f} u, worst seen {float(worst.max() / K.U24):.2f} u")
    assert bool((worst <= fig).all()), float((worst / fig).max())       # the figure covers the worst of the nine combinations, at every x
    assert float(fig.max()) <= 4.0 * float(worst.max())                  # ... and is not slack: at most four times the worst error seen
    for lo in range(-8, 8):                                              # ... on every unit interval of the range as well
        m = (x >= lo) & (x <= lo + 1)
        assert float(fig[m].max()) <= 4.0 * float(worst[m].max()), lo
    # two plain closed forms bound the derived figures from above
    ax = np.abs(x.astype(np.float64))
    assert bool((fig <= ((4 + ax) if act == K.ACT_SIGMOID else (8 + 4 * ax)) * K.U24).all())
    slope = np.abs(np.diff(true) / np.diff(x.astype(np.float64))).max()
    assert slope <= K.LIPSCHITZ[act] * (1 + 1e-6)
