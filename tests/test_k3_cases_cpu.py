"""The construction of the K3 edge tests (tests/k3_cases.py) without the kernel: the reference agrees with real F.grid_sample fed the
reference model's own formula and with the fp32 oracle, both inside the bound the GPU test uses, on every case; each wrong variant of
the lookup, pushed through the same comparator, is rejected; and the touch set pins what a banded cost volume has to hold."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import k3_cases as K

SMALL = tuple(n for n in K.NAMES if K.SPECS[n].B < 100)               # all but the 65535-row case (compared in full where it matters)


def model_formula(cv, disp, radius):
    """CostVolume.__init__ / __call__ and bilinear_sampler of the reference model, restated: pixel coordinates -> [-1, 1] in Python,
    F.grid_sample(align_corners=True) back; level 1 is avg_pool2d over pairs of columns.  fp32 throughout, as the model runs it."""
    B, h, w, _ = cv.shape
    T = 2 * radius + 1
    dx = torch.linspace(-radius, radius, T, dtype=cv.dtype).reshape(1, 1, T, 1)
    img0 = cv.reshape(B * h * w, 1, 1, w)
    img1 = F.avg_pool2d(img0, kernel_size=[1, 2]).reshape(B * h, 1, w, w // 2)
    img0 = img0.reshape(B * h, 1, w, w)
    coords = torch.arange(w, dtype=cv.dtype).expand(B, h, w).reshape(B * h * w, 1, 1, 1)
    d = disp.reshape(B * h * w, 1, 1, 1)

    def sample(img, px, py):
        W = torch.tensor(img.shape[-1], dtype=img.dtype)
        H = torch.tensor(img.shape[-2], dtype=img.dtype)
        grid = torch.cat([2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1], dim=-1)
        return F.grid_sample(img, grid, mode="bilinear", align_corners=True)

    out = []
    for img, x in ((img0, coords - d + dx), (img1, coords / 2 - d / 2 + dx)):
        y = coords + 0 * dx
        s = sample(img, x.reshape(B * h, w, T, 1), y.reshape(B * h, w, T, 1))
        out.append(s.reshape(B, h, w, T).permute(0, 3, 1, 2))
    return out


@pytest.mark.parametrize("dtype", ["float32", "float16"], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", K.NAMES)
def test_reference_vs_grid_sample(name, dtype):
    """the thing cv_lookup.h claims to reproduce, not a restatement of it"""
    c = K.build(name, dtype)
    c1, c2 = model_formula(c.cv, c.disp, c.radius)
    assert c1.dtype == c2.dtype == torch.float32
    res = K.compare(c, K.reference(name, dtype), c1, c2)
    print(K.line(c, "F.grid_sample (CPU, fp32)", res))
    assert not res.bad, "; ".join(res.bad)


@pytest.mark.parametrize("name", K.NAMES)
def test_reference_vs_fp32_oracle(name):
    from oracle import s2m2_oracle as O
    c = K.build(name)
    assert c.w >= 4
    c1, c2 = O.cv_lookup(c.cv, c.disp, c.radius)
    res = K.compare(c, K.reference(name), c1, c2)
    print(K.line(c, "oracle.cv_lookup (fp32)", res))
    assert not res.bad, "; ".join(res.bad)


@pytest.mark.parametrize("variant", K.VARIANTS)
def test_wrong_variants_are_rejected(variant):
    """if one passes, the inputs are too tame"""
    caught = []
    for name in SMALL:
        c = K.build(name)
        res = K.compare(c, K.reference(name), *(torch.from_numpy(np.ascontiguousarray(a)) for a in K.lookup(c.cv, c.disp, c.radius, variant)))
        if res.bad:
            caught.append(name)
    print(f"{variant}: rejected on {len(caught)} of {len(SMALL)} cases")
    assert caught, f"the wrong variant {variant} passes every case"


def test_comparator_takes_every_element_and_the_sign_of_zero():
    name = "w8_r1"
    c, ref = K.build(name), K.reference(name)
    good = [torch.from_numpy(np.ascontiguousarray(a)).float() for a in ref[:2]]
    assert not K.compare(c, ref, *good).bad
    y = c.rows[0].index("zero")
    one = [g.clone() for g in good]
    one[1][0, 1, y, 5] += 40 * 2.0 ** -24 * c.A                           # one element, four bounds off
    res = K.compare(c, ref, *one)
    assert len(res.bad) == 1 and "corr2" in res.bad[0] and '"zero"' in res.bad[0] and "1 elements" in res.bad[0]
    nan = [g.clone() for g in good]
    nan[0][0, 0, 0, 0] = float("nan")
    assert K.compare(c, ref, *nan).bad
    yh = c.rows[0].index("huge")
    assert bool((good[0][0, :, yh] == 0).all()) and bool((good[1][0, :, yh] == 0).all())
    neg = [g.clone() for g in good]
    neg[0][0, 2, yh, 3] = -0.0
    assert any("+0.0" in b for b in K.compare(c, ref, *neg).bad)
    half = [g.half() for g in good]                                      # an fp16 output passes its own bound, not the fp32 one
    assert not K.compare(c, ref, *half, torch.float16).bad and K.compare(c, ref, *half, torch.float32).bad


def test_cases_reach_their_edges():
    """every pattern on every single-image case; the coordinate patterns put x where they say; no disparity is NaN or inf"""
    for name in SMALL:
        c = K.build(name)
        assert bool(torch.isfinite(c.disp).all()) and c.disp.dtype == torch.float32
        if c.B == 1:
            assert c.rows[0] == K.PATTERNS and c.h == len(K.PATTERNS)
    c = K.build("w304_r4")
    i = torch.arange(304.0)
    row = lambda p: c.disp[0, 0, c.rows[0].index(p)]
    assert bool((row("zero") == 0).all()) and bool((i - row("x=0") == 0).all()) and bool((i - row("x=w-1") == 303).all())
    assert bool((row("int") == row("int").floor()).all()) and bool((row("int") <= i).all()) and bool((row("int") >= 0).all())
    assert bool(((row("half") * 2) % 2 == 1).all())
    for p in K.NONNEG:
        assert bool((row(p) >= 0).all()), p
    for p, xt, lvl in (("L0 x=-1", -1, 0), ("L0 x=ws", 304, 0), ("L1 x=-1", -1, 1), ("L1 x=ws-1", 151, 1), ("L1 x=ws", 152, 1)):
        d = row(p)
        x = i - d if lvl == 0 else i / 2 - d / 2
        assert bool((x[0::3] == xt).all())
        exact = i - xt if lvl == 0 else i - 2 * xt
        assert bool((d[1::3] > exact[1::3]).all()) and bool((d[2::3] < exact[2::3]).all())
    big = K.build("B255_h257_w4_r4")
    assert big.B * big.h == 65535 and {p for r in big.rows for p in r} == set(K.PATTERNS)
    two = K.build("B2_h3_w72_r4")
    assert two.B == 2 and two.h == 3 and not torch.equal(two.cv[0], two.cv[1]) and not torch.equal(two.disp[0], two.disp[1])


def test_volume_is_token_like():
    c = K.build("w304_r4")
    assert 120 < c.A < 150
    ridge = c.cv.amax(3)
    assert float(ridge.min()) > 100
    assert 9 < float(c.cv[c.cv < 60].std()) < 13                         # the background
    h = K.build("w304_r4", "float16")
    assert torch.equal(h.cv, h.cv.half().float()) and not torch.equal(h.cv, c.cv)


def _nonneg_rows(name):
    c = K.build(name)
    rows = [(b, y) for b in range(c.B) for y in range(c.h) if c.rows[b][y] in K.NONNEG]
    return c, rows, torch.stack([c.disp[b, 0, y] for b, y in rows])[None, None]


@pytest.mark.parametrize("name", SMALL)
def test_touch_set_of_nonnegative_disparities(name):
    """What a banded cost volume (K1, band >= 0) has to hold for a use_positivity model: on volume row r the lookups of d >= 0 read columns
    j <= r + 2 radius + 4 -- r + 12 at radius 4, one more than "i + 11": pixel i's own row is read up to i + 11 (level 1, d = 0, even i),
    and where the fp32 round trip of the y coordinate lands just below i, row i - 1 is read at the same columns with a weight of 1e-6."""
    c, rows, disp = _nonneg_rows(name)
    assert rows
    reach = 2 * c.radius + 4
    at_reach = []
    for R, i, y, j, level, rowsel in K.touches(disp, c.w, c.radius):
        assert bool((j <= y + reach).all()), (name, level, rowsel, int((j - y).max()))
        m = j == y + reach
        if m.any():
            at_reach.append((level, rowsel))
            assert level == 1 and rowsel == 0 and bool((y[m] == i[m] - 1).all())   # only level-1 reads of row y0 = i - 1
    if name in ("w72_r4", "w304_r4"):
        assert at_reach, "no read at column r + 12: the finding this test pins is gone"
    mask = K.touch_set(disp, c.w, c.radius)[0]
    full = K.reference(name).touch
    for n, (b, y) in enumerate(rows):
        assert np.array_equal(mask[n], full[b, y])
    jj, rr = np.meshgrid(np.arange(c.w), np.arange(c.w))
    assert not mask[:, jj > rr + reach].any()


def test_touch_set_counts_zero_weight_reads_and_skips_row_y1_when_wy_is_zero():
    w, r = 8, 0
    disp = torch.zeros(1, 1, 1, w)
    # pixel 0: iy = 0 exactly, wy = 0: row 1 is not read; x = 0 exactly: column x0 + 1 is read with weight 0 (level 1: columns 2 and 3)
    seen = {}
    for R, i, y, j, level, rowsel in K.touches(disp, w, r):
        m = i == 0
        assert not (rowsel == 1 and m.any()) and bool((y[m] == 0).all())
        if m.any():
            seen.setdefault((level, rowsel), set()).update(j[m].tolist())
    assert seen == {(0, 0): {0, 1}, (1, 0): {0, 1, 2, 3}}
    far = K.touch_set(torch.full((1, 1, 1, w), 1e6), w, r)
    assert not far.any()
