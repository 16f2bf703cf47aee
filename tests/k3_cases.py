"""Token-like cost volumes, adversarial disparity rows, the reference and the comparator of the K3 (s2m2_cv_lookup, csrc/cv_lookup.hip +
csrc/cv_lookup.h) edge tests, shared by tests/test_hip_k3_edges.py (the kernel) and tests/test_k3_cases_cpu.py (the construction itself,
without the kernel: what agrees with F.grid_sample and with the fp32 oracle and rejects a wrong variant on the CPU is literally what
the GPU test asserts).

Volume      what K1 hands to K3: background N(0, 11), a ridge of about 124 along j = i - d_i (d_i piecewise constant), so neighbouring
            columns differ by tens and a coordinate that is off by 1e-5 px costs about 1e-3 -- an order above the bound.  Seeded, built on
            the CPU; for float16 the volume is rounded to fp16 once and kernel and reference read the rounded values.
Disparity   every image row of a case carries ONE pattern (PATTERNS, disparity_row()), so a failure names its pattern: integers, exact
            zeros, x on 0 and on w - 1, half-integers, x on -1 / ws - 1 / ws of either level and one fp32 ulp to both sides, +-1e-6,
            +-1e6 and +-1e30 (every tap is zero padding: the output is +0.0, compared bitwise), uniform.  No NaN, no inf.
Reference   the kernel's COORDINATES are fp32 on purpose: they reproduce the reference model's pixel -> normalised -> pixel round trip
            (`2 x / (W - 1) - 1` in Python, `(g + 1) ((size - 1) / 2)` in grid_sample's CPU kernel, align_corners=True), which lands an
            ulp or so away from x -- a float64 coordinate would be the wrong reference.  So x, ix, iy, x0, y0, wx, wy, ex, ey are numpy
            float32, one IEEE operation per step, in the order of cv_lookup.h (level 1: (i / 2 - d / 2) + dx); the four weights, the
            level-1 pair average and the four-term blend are float64 from those numbers.  Zeros padding and the skip of row y0 + 1
            when wy == 0 are part of it.
Touch set   touch_set(): every volume element lookup_tap dereferences -- reads with weight 0 included (column x0 + 1 when wx == 0), row
            y0 + 1 left out when wy == 0, both columns 2x and 2x + 1 at level 1.
Bound       with identical coordinates the kernel differs from the reference only by fp32 roundings, each at most u = 2^-24 relative:
            per term the level-1 average (a + b) / 2, the weight product and value * weight -- 3 u |term|, and the |term|s add up to at
            most A (ex + wx) (ey + wy) <= A (1 + u)^2 with A = max |cv| -- and the three sums that are not `0 + x`, each of a partial result
            of at most A: 3 u A.  6 u A in all; 8 u A against a reference that took ex = 1 - wx and ey = 1 - wy exactly (this one shares
            their fp32 values with the kernel, as grid_sample does).  BOUND_ULPS = 10.  An fp16 output adds its own rounding,
            2^-11 |ref| + 2^-25 (half an fp16 ulp, and the subnormal step).  Derived, not measured: if a correct kernel exceeds it, a
            rounding is missing above.  Every element is judged.
"""
import collections
import functools
import zlib

import numpy as np
import torch

f32 = np.float32
BOUND_ULPS = 10
TDT = {"float32": torch.float32, "float16": torch.float16}
SHORT = {"float32": "fp32", "float16": "fp16", torch.float32: "fp32", torch.float16: "fp16"}

EDGES = ("L0 x=-1", "L0 x=ws-1", "L0 x=ws", "L1 x=-1", "L1 x=ws-1", "L1 x=ws")
PATTERNS = ("int", "zero", "x=0", "x=w-1", "half") + EDGES + ("tiny", "tiny+", "huge", "uniform", "uniform0i")
NONNEG = ("int", "zero", "x=0", "half", "tiny+", "uniform0i")          # d >= 0 everywhere: what a use_positivity model hands to K3
BAND_PATTERNS = ("zero", "tiny+", "int", "x=0", "uniform0i")            # the rows of the K1 band -> K3 test

Spec = collections.namedtuple("Spec", "w radius B rows")                # rows[b][y]: the pattern of image row (b, y)


def _specs():
    s = {}
    for w in (4, 6, 10, 128, 304, 608):         # 4: smallest legal; 6, 10: odd ws; 128: w * 2T = 9 blocks exactly; 304: grid tail; 608
        s[f"w{w}_r4"] = Spec(w, 4, 1, (PATTERNS,))
    for w in (8, 72):                           # 8: the row is narrower than 2r + 1 at r = 4 and r = 16
        for r in (0, 1, 4, 16):
            s[f"w{w}_r{r}"] = Spec(w, r, 1, (PATTERNS,))
    s["B2_h3_w72_r4"] = Spec(72, 4, 2, (("uniform", "zero", "L1 x=ws"), ("half", "uniform", "int")))
    B, h = 255, 257                             # B * h = 65535: the last legal grid row
    s["B255_h257_w4_r4"] = Spec(4, 4, B, tuple(tuple(PATTERNS[(b * h + y) % len(PATTERNS)] for y in range(h)) for b in range(B)))
    return s


SPECS = _specs()
NAMES = tuple(SPECS)
Case = collections.namedtuple("Case", "name w radius B h dtype rows cv disp A")   # cv (B,h,w,w), disp (B,1,h,w): float32 CPU tensors


def disparity_row(pattern, w, g):
    """the w disparities of one image row, float32"""
    i = torch.arange(w, dtype=torch.float32)
    k = torch.arange(w)
    if pattern == "int":
        return torch.floor(torch.rand(w, generator=g) * (i + 1)).clamp(max=i)
    if pattern == "zero":
        return torch.zeros(w)
    if pattern == "x=0":
        return i.clone()
    if pattern == "x=w-1":
        return i - (w - 1)
    if pattern == "half":
        return torch.floor(torch.rand(w, generator=g) * (i + 1)).clamp(max=i) + 0.5
    if pattern in EDGES:
        level, at = pattern.split(" x=")
        ws = w if level == "L0" else w // 2
        xt = {"-1": -1, "ws-1": ws - 1, "ws": ws}[at]
        d = i - xt if level == "L0" else i - 2 * xt                     # x = i - d, or i / 2 - d / 2, is xt at the centre tap
        up, down = torch.nextafter(d, torch.full_like(d, float("inf"))), torch.nextafter(d, torch.full_like(d, float("-inf")))
        return torch.where(k % 3 == 0, d, torch.where(k % 3 == 1, up, down))
    if pattern == "tiny":
        return torch.where(k % 2 == 0, 1e-6, -1e-6).float()
    if pattern == "tiny+":
        return torch.full((w,), 1e-6)
    if pattern == "huge":
        return torch.tensor([1e6, -1e6, 1e30, -1e30])[k % 4]
    if pattern == "uniform":
        return torch.rand(w, generator=g) * (w + 20) - 10
    if pattern == "uniform0i":
        return torch.rand(w, generator=g) * i
    raise KeyError(pattern)


def volume(B, h, w, g):
    cv = torch.randn(B, h, w, w, generator=g) * 11
    seg = max(2, w // 8)
    d = torch.randint(0, max(2, min(w // 4, 48)), (B, h, -(-w // seg)), generator=g).repeat_interleave(seg, 2)[..., :w]
    col = (torch.arange(w) - d).clamp(0, w - 1)
    return cv.scatter_(3, col[..., None], 124 + 3 * torch.randn(B, h, w, 1, generator=g))


def disparities(rows, w, g):
    return torch.stack([torch.stack([disparity_row(p, w, g) for p in row]) for row in rows])[:, None].contiguous()


@functools.lru_cache(maxsize=None)
def build(name, dtype="float32"):
    """built once per process and shared; nothing may write into it"""
    s = SPECS[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    h = len(s.rows[0])
    cv = volume(s.B, h, s.w, g)
    if dtype == "float16":
        cv = cv.half().float()
    disp = disparities(s.rows, s.w, g)
    assert disp.dtype == torch.float32 and bool(torch.isfinite(disp).all()) and disp.shape == (s.B, 1, h, s.w)
    return Case(name, s.w, s.radius, s.B, h, dtype, s.rows, cv.contiguous(), disp, float(cv.abs().max()))


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
VARIANTS = ("exact_x", "no_half_d", "taps_reversed", "border_clamp", "avg_rows", "transposed", "drop_y1")


def _roundtrip(pix, size):
    g = f32(2) * pix / (size - f32(1)) - f32(1)
    return (g + f32(1)) * ((size - f32(1)) / f32(2))


Piece = collections.namedtuple("Piece", "level rowsel colsel ok y x weight")


def _walk(disp, w, radius, variant=None):
    """the (level, row y0 / y0 + 1, column x0 / x0 + 1) reads of every tap.  ok (R, w, T): the kernel dereferences it; y (w,) and x (R, w, T)
    int64: the element of the level's image; weight (R, w, T) float64.  disp (R, w) float32."""
    assert disp.dtype == f32 and disp.ndim == 2
    i = np.arange(w, dtype=f32)
    dx = np.arange(-radius, radius + 1, dtype=f32)
    if variant == "taps_reversed":
        dx = -dx
    iy = i if variant == "exact_x" else _roundtrip(i, f32(w))
    y0f = np.floor(iy)
    wy = iy - y0f
    ey = f32(1) - wy
    assert iy.dtype == wy.dtype == ey.dtype == f32
    y0 = y0f.astype(np.int64)
    d = disp[:, :, None]
    for level in (0, 1):
        if level == 0:
            x, ws = (i[None, :, None] - d) + dx[None, None, :], w
        elif variant == "no_half_d":
            x, ws = (i[None, :, None] / f32(2) - d) + dx[None, None, :], w // 2
        else:
            x, ws = (i[None, :, None] / f32(2) - d / f32(2)) + dx[None, None, :], w // 2
        ix = x if variant == "exact_x" else _roundtrip(x, f32(ws))
        x0f = np.floor(ix)
        wx = ix - x0f
        ex = f32(1) - wx
        assert x.dtype == ix.dtype == wx.dtype == ex.dtype == f32
        near = (x0f >= f32(-2)) & (x0f <= f32(ws) + f32(1))             # beyond: every tap is zero padding, nothing is read
        x0 = np.where(near, x0f, f32(-4)).astype(np.int64)
        if variant == "border_clamp":
            x0 = np.clip(x0f, -1, ws).astype(np.int64)
        for rowsel in (0, 1):
            if rowsel and variant == "drop_y1":
                continue
            y = y0 + rowsel
            rowok = (y >= 0) & (y < w) & ((wy != 0) if rowsel else np.ones(w, bool))
            wrow = (wy if rowsel else ey).astype(np.float64)
            for colsel in (0, 1):
                xc = x0 + colsel
                if variant == "border_clamp":
                    xc, colok = np.clip(xc, 0, ws - 1), np.ones(xc.shape, bool)
                else:
                    colok = (xc >= 0) & (xc < ws) & near
                wcol = (wx if colsel else ex).astype(np.float64)
                yield Piece(level, rowsel, colsel, colok & rowok[None, :, None], y, xc, wrow[None, :, None] * wcol)


def lookup(cv, disp, radius, variant=None):
    """cv (B,h,w,w), disp (B,1,h,w) float32 tensors -> corr1, corr2 (B,2r+1,h,w) float64 numpy arrays"""
    B, h, w, _ = cv.shape
    T = 2 * radius + 1
    img = cv.reshape(B * h, w, w).numpy()
    if variant == "transposed":
        img = img.transpose(0, 2, 1)
    R = np.arange(B * h)[:, None, None]
    out = [np.zeros((B * h, w, T)), np.zeros((B * h, w, T))]
    with np.errstate(over="ignore", invalid="ignore"):
        for p in _walk(disp.reshape(B * h, w).numpy(), w, radius, variant):
            y = np.clip(p.y, 0, w - 1)[None, :, None]
            ws = w if p.level == 0 else w // 2
            x = np.clip(p.x, 0, ws - 1)
            if p.level == 0:
                val = img[R, y, x].astype(np.float64)
            elif variant == "avg_rows":
                val = (img[R, y, 2 * x].astype(np.float64) + img[R, np.minimum(y + 1, w - 1), 2 * x]) / 2
            else:
                val = (img[R, y, 2 * x].astype(np.float64) + img[R, y, 2 * x + 1]) / 2
            out[p.level] += np.where(p.ok, val * p.weight, 0.0)
    return tuple(o.reshape(B, h, w, T).transpose(0, 3, 1, 2) for o in out)


def touch_set(disp, w, radius):
    """disp (B,1,h,w) float32 tensor -> bool (B,h,w,w) numpy: the volume elements the lookups of these disparities dereference"""
    B, _, h, _ = disp.shape
    touch = np.zeros((B * h, w, w), bool)
    for R, i, y, j, level, rowsel in touches(disp, w, radius):
        touch[R, y, j] = True
    return touch.reshape(B, h, w, w)


def touches(disp, w, radius):
    """the same reads as lists: (image row R, pixel i, volume row y, volume column j) int64 arrays per (level, rowsel) piece"""
    B, _, h, _ = disp.shape
    with np.errstate(over="ignore", invalid="ignore"):
        for p in _walk(disp.reshape(B * h, w).numpy(), w, radius):
            R, i, t = np.nonzero(p.ok)
            y, x = p.y[i], p.x[R, i, t]
            for j in ((x,) if p.level == 0 else (2 * x, 2 * x + 1)):
                yield R, i, y, j, p.level, p.rowsel


Ref = collections.namedtuple("Ref", "c1 c2 touch")


@functools.lru_cache(maxsize=None)
def touch(name):
    c = build(name)
    return touch_set(c.disp, c.w, c.radius)


@functools.lru_cache(maxsize=None)
def reference(name, dtype="float32"):
    """computed once per process and shared"""
    c = build(name, dtype)
    c1, c2 = lookup(c.cv, c.disp, c.radius)
    assert c1.dtype == c2.dtype == np.float64
    return Ref(c1, c2, touch(name))


# ---- the comparator -----------------------------------------------------------------------------------------------------------------------
def bound(A, ref, out_dtype):
    b = BOUND_ULPS * 2.0 ** -24 * A + 0 * np.abs(ref)
    if out_dtype in ("float16", torch.float16):
        b = b + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25
    return b


Result = collections.namedtuple("Result", "ratio1 ratio2 bad")


def compare(case, ref, c1, c2, out_dtype=torch.float32):
    """corr1, corr2 (B,2r+1,h,w) of one run against a Ref (or a (c1, c2) pair): every element within bound(), every tap of a "huge" row
    +0.0 bit for bit.  bad: what fails, with the pattern of the worst image row (empty: the run passes)."""
    bad, ratios = [], []
    huge = np.array([[p == "huge" for p in row] for row in case.rows])                       # (B, h)
    for lvl, (got, want) in enumerate(zip((c1, c2), ref[:2])):
        raw = got.detach().cpu()
        want = want.numpy() if isinstance(want, torch.Tensor) else want
        if tuple(raw.shape) != want.shape:
            bad.append(f"corr{lvl + 1}: shape {tuple(raw.shape)}, expected {want.shape}")
            ratios.append(float("inf"))
            continue
        g = raw.double().numpy()
        ratio = np.abs(g - want) / bound(case.A, want, out_dtype)
        ratio = np.where(np.isfinite(g), ratio, np.inf)                                      # NaN and inf fail whatever they are compared to
        per_row = ratio.max(axis=(1, 3))                                                     # (B, h)
        b, y = np.unravel_index(per_row.argmax(), per_row.shape)
        ratios.append(float(per_row[b, y]))
        if not per_row[b, y] <= 1.0:
            n = int((~(ratio <= 1.0)).sum())
            bad.append(f"corr{lvl + 1}: err / bound {per_row[b, y]:.3g} on image row ({b}, {y}) \"{case.rows[b][y]}\", {n} elements over the bound")
        if huge.any():
            bits = raw.contiguous().view(torch.int16 if raw.dtype == torch.float16 else torch.int32 if raw.dtype == torch.float32 else torch.int64)
            rows = bits.numpy().transpose(0, 2, 1, 3)[huge]                                   # (rows, T, w)
            if rows.any():
                bad.append(f"corr{lvl + 1}: {int((rows != 0).sum())} taps of \"huge\" rows are not +0.0")
    return Result(ratios[0], ratios[1], bad)


def line(case, what, res):
    return (f"{case.name:18s} cv {SHORT[case.dtype]}  {what:34s} err / bound  corr1 {res.ratio1:6.3f}  corr2 {res.ratio2:6.3f}"
            f"   (bound {BOUND_ULPS} * 2^-24 * {case.A:.1f})")
