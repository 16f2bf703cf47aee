"""Cases, inputs, the float64 reference, the elementwise bounds and the one comparator of the K1 (s2m2_cost_volume, csrc/ln_corr.hip) block-shape
tests, shared by tests/test_hip_k1_blocks.py (the kernel through the C ABI) and tests/test_k1_cases_cpu.py (the planner of
csrc/ln_corr_select.h tabulated, a torch emulation of the kernel's arithmetic and deliberately wrong variants of it): what rejects a wrong
variant on the CPU is literally what the GPU test runs.

A case is a shape (B, h, w), a configuration (token dtype, volume dtype, C), a form (LayerNorm inside the kernel / tokens normalised already)
and the launch plan it claims to reach: strips per image row, waves per block, chunks of right tokens, waves past the row end, and whether the
block is the widest the configuration launches.  The plans are literal (PLANS); tests/test_k1_cases_cpu.py asks the planner for every one
of them, so a moved threshold fails there and cannot quietly put these cases back onto two-wave blocks.

Shapes: the smallest at which the planner leaves its strip-splitting loop (B * h >= 200 rows, or blocks that are full already).
  A (2, 100, 304)  one strip of 10 waves (fp16 C <= 256; 2 chunks at TPW = 16), 2 x 5 / 2 x 6 waves with 2 - 4 chunks elsewhere, 3 - 5 strips in fp32
  B (3, 67, 328)   201 rows: no grid is a multiple of 8; 11 column tiles, the last pair a single tile 8 columns wide; 11 waves at C = 128 fp16
  C (1, 100, 608)  the XL width: 2 - 10 strips of full blocks, a wave past the row end in the last strip, 4 - 7 chunks at wide C
  D (1, 200, 72)   3 waves, an odd tile count; 4 waves, one of them past the row end, and a one-tile second chunk at TPW = 16
  E (1, 200, 360)  fp16 tokens at C = 64 only: 12 waves, the widest block of all
  F (1, 200, 280)  9 waves: the widest block of fp16 -> fp32 at C = 128 and of fp32 at C = 64, which A - D do not reach

Inputs: tokens randn * 1.5 + 0.2 per channel; every 37th token has a mean of four standard deviations; every fifth right token is the left
token three pixels on plus noise, as a match is (the volume then holds values near C as well as N(0, sqrt(C))).  Tokens are rounded to the
token dtype first: the reference works on the values the kernel reads.

Reference: float64 layer_norm (biased variance, eps 1e-5, affine) and the batched product, on the device the tokens live on.  No element is
masked.  Bounds, elementwise, from the arithmetic and nothing measured -- a, b the float64 (normalised) tokens, S = sum_k |a_k b_k|:
  accumulation (fp32 MFMA chain, any order)           C * 2^-24 * S
  operands rounded to fp16 (LN form, fp16 tokens)     (2 * 2^-11 + 2^-22) * S
  operands in fp32 (LN form, fp32 tokens)             2 * 2^-24 * S
  LayerNorm computed in fp32 (LN form)                2e-5 * (sum_k |a_k| + sum_k |b_k|)     (TOL_LN of small_kernel_cases.py)
  fp16 volume                                         0.5 * ulp16(ref)
The prenorm form has the accumulation and output terms only: a truncated instead of rounded fp16 volume fails there and nowhere else.
"""
import collections
import functools

import torch

TDT = {"float32": torch.float32, "float16": torch.float16}
SHORT = {"float32": "fp32", "float16": "fp16"}
BYTES = {"float32": 4, "float16": 2}
U24, U11 = 2.0 ** -24, 2.0 ** -11
TOL_LN32 = 2e-5                            # small_kernel_cases.TOL_LN["float32"]
EPS = 1e-5
HIGH_MEAN = 6.0                            # four standard deviations of 1.5
FORMS = ("ln", "pre")
CS = (64, 128, 192, 256, 384)
PAIRS = (("float16", "float16"), ("float16", "float32"), ("float32", "float32"))
CONFIGS = tuple((t, o, C) for t, o in PAIRS for C in CS)

# (token dtype, volume dtype, C) -> (NWMAX, NWGRAN, TPW): csrc/ln_corr_select.h restated (test_k1_cases_cpu.py compares)
BLOCK = {
    ("float16", "float16", 64): (12, 1, 32), ("float16", "float16", 128): (11, 1, 32), ("float16", "float16", 192): (10, 2, 16),
    ("float16", "float16", 256): (10, 2, 16), ("float16", "float16", 384): (8, 2, 16),
    ("float16", "float32", 64): (12, 1, 32), ("float16", "float32", 128): (9, 1, 32), ("float16", "float32", 192): (10, 2, 16),
    ("float16", "float32", 256): (8, 2, 16), ("float16", "float32", 384): (6, 2, 16),
    ("float32", "float32", 64): (9, 1, 32), ("float32", "float32", 128): (6, 1, 32), ("float32", "float32", 192): (4, 1, 32),
    ("float32", "float32", 256): (3, 1, 32), ("float32", "float32", 384): (2, 1, 32),
}

SHAPES = {"A": (2, 100, 304), "B": (3, 67, 328), "C": (1, 100, 608), "D": (1, 200, 72), "E": (1, 200, 360), "F": (1, 200, 280)}

Plan = collections.namedtuple("Plan", "nstrip nw nchunks idle full")     # idle: waves past the row end; full: nw == NWMAX

# shape -> dtype pair -> per C of CS: (nstrip, nw, nchunks, idle waves, nw == NWMAX), tabulated from ln_corr_select.h
_P = {
    "A": {("float16", "float16"): [(1, 10, 1, 0, 0), (1, 10, 1, 0, 0), (1, 10, 2, 0, 1), (1, 10, 2, 0, 1), (2, 6, 4, 2, 0)],
          ("float16", "float32"): [(1, 10, 1, 0, 0), (2, 5, 2, 0, 0), (1, 10, 2, 0, 1), (2, 6, 4, 2, 0), (2, 6, 4, 2, 1)],
          ("float32", "float32"): [(2, 5, 2, 0, 0), (2, 5, 2, 0, 0), (3, 4, 3, 2, 1), (4, 3, 4, 2, 1), (5, 2, 5, 0, 1)]},
    "B": {("float16", "float16"): [(1, 11, 1, 0, 0), (1, 11, 1, 0, 1), (2, 6, 4, 1, 0), (2, 6, 4, 1, 0), (2, 6, 4, 1, 0)],
          ("float16", "float32"): [(1, 11, 1, 0, 0), (2, 6, 2, 1, 0), (2, 6, 4, 1, 0), (2, 6, 4, 1, 0), (2, 6, 4, 1, 1)],
          ("float32", "float32"): [(2, 6, 2, 1, 0), (2, 6, 2, 1, 1), (3, 4, 3, 1, 1), (4, 3, 4, 1, 1), (6, 2, 6, 1, 1)]},
    "C": {("float16", "float16"): [(2, 10, 2, 1, 0), (2, 10, 2, 1, 0), (2, 10, 4, 1, 1), (2, 10, 4, 1, 1), (3, 8, 5, 5, 1)],
          ("float16", "float32"): [(2, 10, 2, 1, 0), (3, 7, 3, 2, 0), (2, 10, 4, 1, 1), (3, 8, 5, 5, 1), (4, 6, 7, 5, 1)],
          ("float32", "float32"): [(3, 7, 3, 2, 0), (4, 5, 4, 1, 0), (5, 4, 5, 1, 1), (7, 3, 7, 2, 1), (10, 2, 10, 1, 1)]},
    "D": {("float16", "float16"): [(1, 3, 1, 0, 0), (1, 3, 1, 0, 0), (1, 4, 2, 1, 0), (1, 4, 2, 1, 0), (1, 4, 2, 1, 0)],
          ("float16", "float32"): [(1, 3, 1, 0, 0), (1, 3, 1, 0, 0), (1, 4, 2, 1, 0), (1, 4, 2, 1, 0), (1, 4, 2, 1, 0)],
          ("float32", "float32"): [(1, 3, 1, 0, 0), (1, 3, 1, 0, 0), (1, 3, 1, 0, 0), (1, 3, 1, 0, 1), (2, 2, 2, 1, 1)]},
    "E": {("float16", "float16"): [(1, 12, 1, 0, 1)], ("float16", "float32"): [(1, 12, 1, 0, 1)]},
    "F": {("float16", "float32"): [None, (1, 9, 1, 0, 1)], ("float32", "float32"): [(1, 9, 1, 0, 1)]},
}
PLANS = {(s, t, o, C): Plan(*p) for s, by_pair in _P.items() for (t, o), ps in by_pair.items() for C, p in zip(CS, ps) if p}


class Case(collections.namedtuple("Case", "shape tdt cdt C form plan")):
    @property
    def id(self):
        return f"{self.shape}-{SHORT[self.tdt]}-{SHORT[self.cdt]}-C{self.C}-{self.form}"

    @property
    def dims(self):
        return SHAPES[self.shape]

    @property
    def tpw(self):
        return BLOCK[(self.tdt, self.cdt, self.C)][2]

    @property
    def tj(self):
        """right tokens per chunk"""
        return self.plan.nw * self.tpw


@functools.lru_cache(maxsize=None)
def all_cases():
    """ordered so that the cases that share tokens and a reference (same shape, token dtype, C and form) follow one another"""
    keys = sorted(PLANS, key=lambda k: (k[0], k[1], k[3], k[2]))
    return tuple(Case(s, t, o, C, form, PLANS[(s, t, o, C)]) for s, t, o, C in keys for form in FORMS)


def cases(shapes=None, pairs=None, Cs=None, forms=None):
    return [c for c in all_cases() if (shapes is None or c.shape in shapes) and (pairs is None or (c.tdt, c.cdt) in pairs)
            and (Cs is None or c.C in Cs) and (forms is None or c.form in forms)]


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
Inputs = collections.namedtuple("Inputs", "tokens gamma beta B")         # tokens (2B, h, w, C) in the token dtype; gamma, beta fp32


@functools.lru_cache(maxsize=2)
def inputs(shape, tdt, C, device="cpu", rows=None):
    """built once and shared by the cases that read them; nothing may write into them.  rows = (B, h) overrides the shape's (the CPU tests run
    the emulation on fewer image rows: the planner is not involved there)"""
    B, h, w = SHAPES[shape]
    if rows:
        B, h = rows
    g = torch.Generator(device=device).manual_seed(w * 1000 + C + (tdt == "float16"))
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    tok = rn(2 * B, h, w, C) * 1.5 + 0.2
    j = torch.arange(2, w, 5, device=device)                                        # every fifth right token is a match
    tok[B:, :, j] = tok[:B, :, (j + 3) % w] + 0.1 * rn(B, h, j.numel(), C)
    tok[:, :, 5::37] += HIGH_MEAN                                                  # (left and right, matches among them)
    gamma = 1 + 0.1 * rn(C)
    beta = 0.05 * rn(C)
    return Inputs(tok.to(TDT[tdt]).contiguous(), gamma, beta, B)


# ---- reference and bound ------------------------------------------------------------------------------------------------------------------
def layer_norm64(x, gamma, beta):
    """float64: biased variance, eps 1e-5, affine"""
    assert x.dtype == torch.float64
    d = x - x.mean(-1, keepdim=True)
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + EPS) * gamma.double() + beta.double()


def operands(inp, form):
    """a (B, h, w, C), b (B, h, w, C) in float64: what the product is taken of"""
    x = inp.tokens.double()
    if form == "ln":
        x = layer_norm64(x, inp.gamma, inp.beta)
    return x[:inp.B], x[inp.B:]


def product64(a, b):
    """cv[b, y, i, j] = <a[b, y, i], b[b, y, j]>"""
    return torch.matmul(a, b.transpose(-1, -2))


def ulp16(ref):
    """spacing of fp16 at |ref| (2^-24 below the normal range)"""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def bound(a, b, ref, tdt, cdt, C, form):
    S = product64(a.abs(), b.abs())
    bnd = C * U24 * S
    if form == "ln":
        bnd = bnd + ((2 * U11 + U11 * U11) if tdt == "float16" else 2 * U24) * S
        bnd = bnd + TOL_LN32 * (a.abs().sum(-1)[..., :, None] + b.abs().sum(-1)[..., None, :])
    if cdt == "float16":
        bnd = bnd + 0.5 * ulp16(ref)
    return bnd


Ref = collections.namedtuple("Ref", "cv bound")


@functools.lru_cache(maxsize=2)
def _ref_ab(shape, tdt, C, form, device, rows):
    a, b = operands(inputs(shape, tdt, C, device, rows), form)
    ref = product64(a, b)
    assert ref.dtype == torch.float64
    return a, b, ref


def reference(case, device="cpu", rows=None):
    a, b, ref = _ref_ab(case.shape, case.tdt, case.C, case.form, device, rows)
    return Ref(ref, bound(a, b, ref, case.tdt, case.cdt, case.C, case.form))


# ---- comparator ---------------------------------------------------------------------------------------------------------------------------
Result = collections.namedtuple("Result", "err bound ratio nbad n where")


def compare(out, ref, where=None):
    """out against Ref, elementwise, on every element (or those of the boolean mask ``where``): the element of the worst error / bound.  An
    element that is not finite (the NaN prefill of a buffer: never written) has ratio inf."""
    o = out.detach().double()
    assert o.shape == ref.cv.shape, (o.shape, ref.cv.shape)
    err = (o - ref.cv).abs()
    ratio = torch.where(torch.isfinite(err), err / ref.bound, torch.full_like(err, float("inf")))
    if where is not None:
        ratio = torch.where(where, ratio, torch.zeros_like(ratio))
    k = int(ratio.argmax())
    n = int(where.sum()) if where is not None else ratio.numel()
    return Result(float(err.flatten()[k]), float(ref.bound.flatten()[k]), float(ratio.flatten()[k]), int((ratio > 1).sum()), n,
                  tuple(int(v) for v in torch.unravel_index(torch.tensor(k), ratio.shape)))


def line(case, res, note=""):
    p = case.plan
    B, h, w = case.dims
    return (f"{case.id:24s} B{B} h{h:3d} w{w:3d}  {p.nstrip:2d} x {p.nw:2d} waves{'=max' if p.full else '    '} chunks {p.nchunks:2d} idle {p.idle}"
            f"  max err {res.err:.3e}  bound {res.bound:.3e}  ratio {res.ratio:.3f}  over 1: {res.nbad} of {res.n}  "
            f"{'ok' if res.ratio <= 1 else 'FAIL'}{note}")


# ---- band ---------------------------------------------------------------------------------------------------------------------------------
def band_masks(case, band, device="cpu"):
    """(inside, beyond), both (w, w) bool: inside = j <= i + band, what a banded launch must get right; beyond = the columns the kernel's own
    rule leaves alone.  A wave owns rows i0 .. i0 + 31 and walks chunks of case.tj columns from jbase; in a chunk it stores whole pairs of
    32-column tiles and stops after (i0 + 31 + band - jbase) / 64 + 1 of them (none when that column lies before the chunk), so it writes
    columns jbase .. jbase + 64 * pairs - 1.  Where a chunk has an odd number of tiles its last pair reaches 32 columns into the next chunk:
    the full launch overwrites them there, a banded launch whose band ends inside that pair leaves a copy of the chunk's last tile in them
    -- beyond the band, before the limit."""
    w, tj = case.dims[2], case.tj
    i = torch.arange(w, device=device)[:, None]
    j = torch.arange(w, device=device)[None, :]
    written = torch.zeros(w, w, dtype=torch.bool, device=device)
    for jbase in range(0, w, tj):
        ntile = min((w - jbase + 31) // 32, tj // 32)
        last = (i | 31) + band - jbase
        pairs = torch.where(last < 0, torch.zeros_like(last), last // 64 + 1).clamp(max=(ntile + 1) // 2)
        written |= (j >= jbase) & (j < jbase + 64 * pairs)
    return j <= i + band, ~written
