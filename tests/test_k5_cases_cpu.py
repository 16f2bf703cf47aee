"""The construction of the K5 strided tests (tests/k5_cases.py) without the kernel: the float64 reference agrees with torch's own fp32
F.conv2d inside the bound the GPU test uses, the `exact` cases are representable in both I/O dtypes, the comparator takes the rounded
reference and nothing one element away from it, each of the eight wrong loaders is rejected wherever it differs by construction (and on
an `exact` case by a changed integer), the GELU figures the bound quotes hold for the header's formulas, and K order 1 as pack.pack_conv
lays it out multiplies out to the same layer when the K cursor of csrc/conv.hip walks it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import k5_cases as K
from s2m2_amd import pack

DTYPES = ("float32", "float16")
IDS = ("fp32", "fp16")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", K.NAMES)
def test_reference_vs_torch_fp32(name, dtype):
    """torch's fp32 convolution of the same operands, pushed through the comparator the kernel faces"""
    c, ref = K.build(name, dtype), K.reference(name, dtype)
    L = c.layer
    x = torch.cat(c.xs, -1).permute(0, 3, 1, 2)
    pre = F.conv2d(x, c.w, c.b, stride=L.stride, padding=(L.KH // 2, L.KW // 2)).permute(0, 2, 3, 1)
    assert pre.dtype == torch.float32 and tuple(pre.shape) == (c.N, c.Ho, c.Wo, L.Cout)
    res = K.compare(c, ref, K.finish(c, pre.double()) + 0.0)            # (+ 0.0: the sign of a zero is the kernel's to get right, not torch's)
    print(K.line(c, "F.conv2d (fp32)", res))
    assert not res.bad, "; ".join(res.bad)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_cases_are_representable(dtype):
    names = [n for n in K.NAMES if K.SPECS[n].regime == "exact"]
    assert len(names) >= 40
    for name in names:
        c, ref = K.build(name, dtype), K.reference(name, dtype)
        assert ref.bound is None
        S = K._conv64([x.abs() for x in c.xs], c.w.abs(), c.layer) + c.b.abs().double()
        assert float(S.max()) <= K.EXACT_MAX, name                       # every partial sum, in any order, is an integer of at most 2048
        for t in c.xs + (c.w, c.b):
            assert torch.equal(t, t.round()) and torch.equal(t.to(K.TDT[dtype]).float(), t)
        assert torch.equal(ref.out, ref.out.round()) and torch.equal(ref.out.to(K.TDT[dtype]).double(), ref.out), name
        assert all(bool((x != 0).all()) for x in c.xs)                   # a tap read where zero padding belongs always changes a product
        assert float(ref.out.abs().max()) > 8, name                      # (not a layer of zeros)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", K.NAMES)
def test_comparator_accepts_the_rounded_reference(name, dtype):
    c, ref = K.build(name, dtype), K.reference(name, dtype)
    res = K.compare(c, ref, ref.out.to(K.TDT[dtype]))
    assert not res.bad and res.ratio <= (0.0 if ref.bound is None else 1.0), res


@pytest.mark.parametrize("name", ["3x3s2_128-3x11x15-exact", "3x3s2_128-3x11x15-gauss-none-x0.5", "5x5s2_16_64-1x33x61-gauss-gelu"])
def test_comparator_judges_every_element(name):
    for dtype in DTYPES:
        c, ref = K.build(name, dtype), K.reference(name, dtype)
        good = ref.out.to(K.TDT[dtype])
        at = (c.N - 1, c.Ho - 1, c.Wo // 2, 5)
        one = good.clone().double()
        one[at] += 1.0 if ref.bound is None else 2.5 * float(ref.bound[at])
        res = K.compare(c, ref, one)
        assert len(res.bad) == 1 and res.where == at and res.bad[0].startswith("1 elements"), res
        nan = good.clone()
        nan[0, 0, 0, 0] = float("nan")
        assert K.compare(c, ref, nan).where == (0, 0, 0, 0) and K.compare(c, ref, nan).bad
        assert K.compare(c, ref, good[:, :-1]).bad and K.compare(c, ref, good[..., :-8]).bad        # a shape is not negotiable
        if ref.bound is None and bool((ref.out == 0).any()):
            neg = good.clone()
            z = tuple(int(i) for i in (ref.out == 0).nonzero()[0])
            neg[z] = -0.0
            assert K.compare(c, ref, neg).where == z and K.compare(c, ref, neg).bad
    c16, c32 = K.build(name, "float16"), K.build(name, "float32")
    if c16.spec.regime == "gauss":                                      # an fp16 result passes its own bound, not the fp32 one
        assert K.compare(c32, K.reference(name, "float32"), K.reference(name, "float32").out.half()).bad


@pytest.mark.parametrize("name", K.SMALL)
def test_the_gather_is_the_layer(name):
    """wrong(case, None) -- the flat index, the tap offset and the mask of the loader -- is F.conv2d"""
    c, ref = K.build(name, "float32"), K.reference(name, "float32")
    got = K.wrong(c)
    if ref.bound is None:
        assert torch.equal(got, ref.out)
    else:
        assert float((got - ref.out).abs().max()) <= 1e-12 * max(1.0, float(ref.out.abs().max()))


@pytest.mark.parametrize("variant", K.VARIANTS)
def test_wrong_variants_are_rejected(variant):
    """on every case where the variant differs by construction, in both dtypes (K order 1 has another chunk per dtype); where it does not,
    it is the layer and passes.  If a differing one passes, the inputs are too tame."""
    exact, total = 0, 0
    for name in K.SMALL:
        for dtype in DTYPES:
            c, ref = K.build(name, dtype), K.reference(name, dtype)
            res = K.compare(c, ref, K.wrong(c, variant))
            if K.differs(c, variant):
                total += 1
                exact += ref.bound is None
                assert res.bad, f"the wrong variant {variant} passes {name} {dtype}"
            else:
                assert not res.bad, f"{variant} is said not to differ on {name} {dtype}: {res.bad}"
    print(f"{variant}: rejected on {total} (case, dtype) pairs, {exact} of them bit for bit")
    assert exact >= 1


def test_cases_cover_what_they_claim():
    by = lambda layer, regime=None: {K.SPECS[n].shape for n in K.NAMES if K.SPECS[n].layer == layer and regime in (None, K.SPECS[n].regime)}
    assert by("3x3s2_128", "exact") >= set(K.SHAPES) and by("5x5s2_16_64", "exact") >= set(K.SHAPES)
    assert {K.SPECS[n].layer for n in K.NAMES} == set(K.LAYERS)
    assert {K.SPECS[n].epi for n in K.NAMES} == {0, 1, 2, 3, 4} and {K.SPECS[n].act for n in K.NAMES} == {0, 1, 2}
    assert any(K.SPECS[n].scale == 0.5 for n in K.NAMES)
    M = lambda s: s[0] * -(-s[1] // 2) * -(-s[2] // 2)
    assert [M(s) for s in K.SHAPES[-3:]] == [144, 128, 527] and all(M(s) < 64 for s in K.SHAPES[:-3])
    assert -(-M(K.T20_ABOVE) // 128) == 304 and -(-M(K.T20_BELOW) // 128) == 296      # t20_min = 300 lies between
    assert K.LAYERS["5x5s2_16_64"].KH * K.LAYERS["5x5s2_16_64"].KW * 16 == 400         # ends inside a K tile of 32 or 64
    two = K.build("3x3s2_8+128-3x11x15-exact")
    assert K.wide(two, 0).shape[-1] != K.wide(two, 1).shape[-1]
    big = K.wide(two, 1)
    assert bool(torch.isnan(big[0]).all()) and bool(torch.isnan(big[-1]).all()) and bool(torch.isnan(big[..., :K.PAD]).all())
    assert bool(torch.isnan(big[..., -K.PAD:]).all()) and torch.equal(big[1:-1, :, :, K.PAD:-K.PAD], two.xs[1])
    for n in K.NAMES:
        s = K.SPECS[n]
        assert set(s.tiles) <= set(K.TILES) and 0 in s.tiles
        if s.regime == "gauss":
            assert abs(float(torch.cat(K.build(n).xs, -1).mean()) - 0.3) < 0.2 or K.build(n).xs[0].numel() < 500


def test_gelu_figures_of_the_header_hold_where_the_bound_uses_them():
    """csrc/epilogue.h: fast_gelu (fp32 destinations) absolute 3.3e-7, fast_gelu16 absolute 8.1e-7, both restated in numpy float32 by
    tests/test_gelu16_cpu.py; the bound quotes them on [-8, 8], which reference() asserts the GELU cases stay inside"""
    from scipy.special import ndtr
    import test_gelu16_cpu as G
    x = np.linspace(-K.GELU_RANGE, K.GELU_RANGE, 1_000_001).astype(np.float32)
    ref = x.astype(np.float64) * ndtr(x.astype(np.float64))
    # to the two digits the header prints (this restatement rounds after every step, the device fuses its multiply-adds: 3.31e-7 here)
    assert np.abs(G._gelu_as(x) - ref).max() < K.GELU_ABS["float32"] + 0.05e-7
    assert np.abs(G._gelu16(x, G._coefficients()) - ref).max() < K.GELU_ABS["float16"] + 0.05e-7
    slope = np.abs(np.diff(ref) / np.diff(x.astype(np.float64))).max()
    assert slope <= K.LIPSCHITZ[K.ACT_GELU]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kh,kw,cin", [(5, 5, 32), (3, 3, 64), (5, 5, 16)])
def test_korder1_packing_multiplies_out_to_the_same_layer(kh, kw, cin, dtype):
    """the packed weight of either K order times the operand rows gathered in the order KCursor walks them (both K-tile widths of the v1
    and v2 loaders) is the layer, exactly, on small integers; 5x5 on 16 channels has K = 400 and exists in K order 1 in fp32 only"""
    tdt = K.TDT[dtype]
    ch, vec = pack.chunk_channels(tdt), 16 // torch.empty((), dtype=tdt).element_size()
    g = torch.Generator().manual_seed(kh * 100 + cin)
    N, H, W, cout = 2, 5, 6, 16
    x = torch.randint(-2, 3, (N, H, W, cin), generator=g).double()
    w = torch.randint(-2, 3, (cout, cin, kh, kw), generator=g).double()
    ref = F.conv2d(x.permute(0, 3, 1, 2), w, padding=(kh // 2, kw // 2)).permute(0, 2, 3, 1).reshape(-1, cout)
    xp = F.pad(x, (0, 0, kw // 2, kw // 2, kh // 2, kh // 2))            # (N, H + 2 ph, W + 2 pw, cin)
    outs = []
    for korder in (0, 1):
        if korder and cin % ch:
            with pytest.raises(AssertionError):
                pack.pack_conv(w, tdt, korder=1)
            continue
        wp = pack.pack_conv(w, tdt, korder=korder).double()
        assert tuple(wp.shape) == (cout, kh * kw * cin)
        for bk in (4 * vec, 8 * vec):                                   # 64- and 128-byte K rows
            order = K.kcursor(kh, kw, cin, ch, bk, vec, korder)
            assert sorted(map(tuple, order.tolist())) == sorted((a, b, c) for a in range(kh) for b in range(kw) for c in range(cin))
            cols = [xp[:, a:a + H, b:b + W, c] for a, b, c in order.tolist()]
            A = torch.stack(cols, -1).reshape(-1, kh * kw * cin)
            outs.append(A @ wp.T)
            assert torch.equal(outs[-1], ref), (korder, bk)
    assert len(outs) in (2, 4)
