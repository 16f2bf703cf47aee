"""Token-like cost volumes, the float64 reference and the comparator of the K2 (s2m2_sinkhorn_regress) edge tests, shared by
tests/test_hip_k2_edges.py (the kernel through the C ABI) and tests/test_k2_cases_cpu.py (the construction itself, without the kernel:
what passes the fp32 oracle and rejects a wrong variant on the CPU is literally what the GPU test runs).

The volume is what K1 hands to K2: <LN(f0), LN(f1)> of 128-channel tokens with no 1/sqrt(C).  A match scores about 124, a non-match is
N(0, 11), so one column of the volume spans 150 and more -- the seeded ``randn * 3 + 110`` volumes of tests/test_hip_dispinit.py span 35.
  right tokens   layer_norm(randn(B, h, w, 128))
  left token i   layer_norm(right token (i - d_i) + 0.25 * randn); d_i is piecewise constant (segments of w / 8 pixels, values below
                 min(w / 4, 48)) like a real disparity map, so claims on a column collide, and columns stay without a claim, at the steps
                 only.  The column is clamped to >= 0 under positivity (where d_i <= i / 2) and wrapped modulo w without it
  occlusion      about 5 % of the left pixels are unrelated tokens: the dustbin should take them
  planted        matches where the kernel's column mapping has an edge (plants()); a plant and its neighbours share the disparity; any
                 other claim on a plant's column is weakened to about 90 (a "rival": it loses the column and goes to the dustbin); the two
                 plants on column 0 lie on different image rows (h >= 2)
  w <= 16        one pixel of a two-row case is more than the 5 % cap, so nothing is left to chance: zero disparity, no random occlusion,
                 and a column without a claim is unlike every row that sees it (see build())
  fp16           the volume is rounded to fp16 once; kernel and reference read the rounded values

Reference: oracle.s2m2_oracle.sinkhorn_prob / regress on cv.double().  Their constants are fp32 tensors (the log marginals), promoted, so
every tensor stays float64 (asserted); a log marginal rounded to fp32 is off by < 5e-7.

A pixel is "sure" when the reference's top-2 gap exceeds 1e-4 * top1 (the rule of tests/test_hip_dispinit.py) and top1 is a normal fp32
number (_outputs()); at most NOT_SURE_CAP of the pixels may fail it.  Bounds (those of test_sinkhorn_wide_rows_vs_oracle): conf, occ < 5e-5;
disp < 2e-4 + 2e-7 * w where conf >= 1e-2, and tol_disp_low() below that.
"""
import collections
import functools

import torch
import torch.nn.functional as F

C = 128
NOISE = 0.25
RIVAL_NOISE = 1.0
OCCLUDED = 0.05
NOT_SURE_CAP = 0.05
TAIL = 64                                  # under positivity the last TAIL columns meet fewer than TAIL rows
SMALL = 16                                 # up to here one pixel of a two-row case is more than the cap: zero disparity, no random occlusion
TOL_CONF = 5e-5
TOL_OCC = 5e-5
TDT = {"float32": torch.float32, "float16": torch.float16}
SHORT = {"float32": "fp32", "float16": "fp16"}

# every width the GPU test runs at h = 2, B = 1 (both dtypes, positivity on and off)
WIDTHS = (8, 16, 128, 136, 256, 264, 272, 360, 368, 384, 512, 520, 1024, 1032, 1536)


def tol_disp(w):
    return 2e-4 + 2e-7 * w


# ---- the dispatch of s2m2_amd/csrc/sinkhorn.hip, restated (dispatch_ppl, launch_sinkhorn, K2Lds) -----------------------------------------
def lanes(w):
    """lanes per row (GL)"""
    return 16 if w <= 384 else 32 if w <= 768 else 64


def chunk_width(w):
    """columns per chunk: a lane owns 8 consecutive columns in each chunk"""
    return 8 * lanes(w)


def chunks(w):
    return -(-w // chunk_width(w))


def tri_bytes(w, dtype):
    """dynamic LDS of the TRI form: the vectors, the masked triangle, the dustbin row and the -inf piece"""
    gl, nch = lanes(w), chunks(w)
    nwv = 16 if nch == 1 else 8
    vec = 8 if dtype == "float16" else 4
    ns = (w + 4) & ~3
    nvs = max(ns, nch * 8 * gl + 8)
    vec_bytes = ((1 + 2 * nwv) * ns + 4 + nvs) * 4
    q, rem = divmod(w, vec)
    pieces = w + vec * (q * (q - 1) // 2) + q * rem + w // vec + 1
    return ((vec_bytes + 15) & ~15) + pieces * 16


def uses_tri(w, dtype, pos, switch_on=True):
    """the launch keeps the masked triangle in LDS: 16-lane classes, positivity, S2M2_K2_TRI not 0, 160 KB"""
    return bool(pos) and switch_on and lanes(w) == 16 and tri_bytes(w, dtype) <= 160 * 1024


def dispatch_class(w, dtype, pos, switch_on=True):
    return (lanes(w), chunks(w), uses_tri(w, dtype, pos, switch_on))


# ---- the volume ---------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "w h B pos dtype cv planted")     # cv (B, h, w, w) float32 CPU, fp16-exact for float16


def plants(w, h):
    """(image row, pixel, column) of the planted matches.  Image rows alternate so that the two claims on column 0 lie on different rows."""
    cw = chunk_width(w)
    pc = [(0, 0), (1, 0), (w - 1, w - 1)]                                # column 0; column 0 from pixel 1; the diagonal at the last column
    if w > cw:                                                           # the 5-tap window straddles the edge between chunks 0 and 1
        pc += [(min(cw - 1 + 3, w - 2), cw - 1), (min(cw + 3 + 1, w - 3), cw)]
    out, seen = [], set()
    for k, (i, j) in enumerate(pc):
        if i < 0 or j > i or (k % h, i) in seen:
            continue
        seen.add((k % h, i))
        out.append((k % h, i, j))
    return out


def _seed(w, h, B, pos, dtype):
    return ((w * 31 + h) * 7 + B) * 4 + 2 * int(bool(pos)) + (dtype == "float16")


@functools.lru_cache(maxsize=None)
def build(w, pos, dtype, h=2, B=1):
    """built once per process and shared; nothing may write into it"""
    assert h >= 2 and w % 8 == 0
    g = torch.Generator().manual_seed(_seed(w, h, B, pos, dtype))
    ln = lambda t: F.layer_norm(t, (C,))
    right = ln(torch.randn(B, h, w, C, generator=g))
    seg = max(4, w // 8)                                                 # piecewise constant disparity: claims collide at the steps only
    nseg = -(-w // seg)
    d = torch.randint(0, max(2, min(w // 4, 48)), (B, h, nseg), generator=g).repeat_interleave(seg, 2)[..., :w]
    if w <= SMALL:
        d.zero_()
    if pos:
        d = torch.minimum(d, torch.arange(w) // 2)                       # no pile of claims on column 0 at the left edge
    col = torch.arange(w)[None, None, :] - d
    col = col.clamp_min(0) if pos else col % w
    planted = plants(w, h)
    rival = torch.zeros(B, h, w, dtype=torch.bool)                       # another claim on a planted column: weakened below
    for y, i, j in planted:
        rival[:, y] |= col[:, y] == j
    reach = 1 if w <= SMALL else 8                                       # a plant and its neighbours share the disparity: no column is vacated
    for near in (True, False):                                           # next to it (the plants themselves last: they win an overlap)
        for y, i, j in planted:
            for k in (range(i - reach, i + reach + 1) if near else (i,)):
                if 0 <= k < w and 0 <= j + k - i < w:
                    col[:, y, k] = j + k - i
                    rival[:, y, k] = False
    occluded = torch.rand(B, h, w, generator=g) < (OCCLUDED if w > SMALL else 0.0)
    for y, i, _ in planted:
        occluded[:, y, i] = False
    # A column nobody claims takes half of one of the rows that see it (both columns then draw all their mass from that row: a tie to
    # 1e-4 that three sweeps do not resolve) -- one of n rows at random.  Where n is small that row is too often a plant (under
    # positivity only rows >= j see column j), and on a narrow volume one tied pixel is over the cap.  Such a column (any on a narrow
    # volume, the last TAIL under positivity) is a right pixel unlike its surroundings: about -128 / sqrt(n) against the rows that see it.
    orphan = torch.zeros(B, h, w, dtype=torch.bool)
    live = ~(rival | occluded)
    anti = torch.zeros(B, h, w, C)
    for b in range(B):
        for y in range(h):
            claimed = torch.zeros(w, dtype=torch.bool)
            claimed[col[b, y][live[b, y]]] = True
            for j in (~claimed).nonzero()[:, 0].tolist():
                if w <= SMALL or (pos and j >= w - TAIL):
                    rows = live[b, y].clone()
                    rows[:j if pos else 0] = False
                    orphan[b, y, j] = True
                    anti[b, y, j] = -right[b, y, col[b, y][rows]].sum(0)
    right = torch.where(orphan[..., None], ln(anti + NOISE * torch.randn(B, h, w, C, generator=g)), right)
    # a rival is a weaker second claim on the plant's column (about 90 against the plant's 124): it loses the column by e^-34, the dustbin
    # takes it, and its row of the plan stays inside the fp32 range
    strength = torch.where(rival, RIVAL_NOISE, NOISE)[..., None]
    left = ln(torch.gather(right, 2, col[..., None].expand(B, h, w, C)) + strength * torch.randn(B, h, w, C, generator=g))
    left = torch.where(occluded[..., None], ln(torch.randn(B, h, w, C, generator=g)), left)
    cv = torch.einsum("bhic,bhjc->bhij", left, right)
    if dtype == "float16":
        cv = cv.half().float()
    return Case(w, h, B, bool(pos), dtype, cv.contiguous(), tuple(planted))


def column_range(cv, pos):
    """largest max - min over the rows i a column j of one image row meets (under positivity: i >= j)"""
    w = cv.shape[-1]
    if pos:
        upper = torch.ones(w, w, dtype=torch.bool).triu(1)
        hi = cv.masked_fill(upper, float("-inf")).amax(2)
        lo = cv.masked_fill(upper, float("inf")).amin(2)
    else:
        hi, lo = cv.amax(2), cv.amin(2)
    return float((hi - lo).max())


# ---- references ---------------------------------------------------------------------------------------------------------------------------
Ref = collections.namedtuple("Ref", "disp conf occ ind sure top1")      # disp, conf, occ (B, h, w); ind int64; sure bool
FP32_TINY = 2.0 ** -126                   # smallest normal fp32 number
CONF_WELL = 1e-2                          # see check(): where disp is well conditioned
MARGIN = 3.0                              # see check()


def _outputs(cv, pos, ot_iter):
    from oracle import s2m2_oracle as O
    P = O.sinkhorn_prob(cv, pos, ot_iter)
    disp, conf, occ, ind = O.regress(P)
    top = P.topk(2, 3).values
    # The plan is an fp32 tensor in the model (and in K2): a row whose largest entry is no normal fp32 number (the dustbin took the pixel:
    # 1e-45 ... 1e-75 on these volumes) has no argmax there -- the oracle in fp32 answers 0 on such a row.  Float64 separates its entries,
    # fp32 cannot, so such a pixel is not "sure"; it counts towards NOT_SURE_CAP like every other one.
    sure = ((top[..., 0] - top[..., 1]) > 1e-4 * top[..., 0]) & (top[..., 0] >= FP32_TINY)
    assert P.dtype == disp.dtype == conf.dtype == occ.dtype == cv.dtype, (P.dtype, disp.dtype, conf.dtype, occ.dtype)
    return Ref(disp[:, 0], conf[:, 0], occ[:, 0], ind, sure, top[..., 0])


@functools.lru_cache(maxsize=None)
def reference(w, pos, dtype, h=2, B=1, ot_iter=3):
    """float64 throughout, on the values the kernel reads; computed once per process and shared"""
    ref = _outputs(build(w, pos, dtype, h, B).cv.double(), pos, ot_iter)
    assert ref.disp.dtype == ref.conf.dtype == ref.occ.dtype == ref.top1.dtype == torch.float64
    return ref


def oracle_fp32(w, pos, dtype, h=2, B=1, ot_iter=3):
    """the same oracle in its own fp32: what fp32 arithmetic in the model's order of operations reaches on a case"""
    o = _outputs(build(w, pos, dtype, h, B).cv, pos, ot_iter)
    return o.disp, o.conf, o.occ, o.ind


Errors = collections.namedtuple("Errors", "not_sure sure_mismatch planted_mismatch agree conf disp disp_low occ occ_min occ_max finite")


def compare(case, ref, disp, conf, occ, ind):
    """one set of outputs against a Ref: argmax on sure and planted pixels, conf / disp where the argmax agrees (disp apart for pixels of
    conf >= CONF_WELL and below), occ everywhere"""
    disp, conf, occ = (t.detach().cpu().double().reshape(ref.disp.shape) for t in (disp, conf, occ))
    same = ind.detach().cpu().reshape(ref.ind.shape).long() == ref.ind
    planted = torch.zeros_like(same)
    for y, i, j in case.planted:
        planted[:, y, i] = True
    finite = all(bool(torch.isfinite(t).all()) for t in (disp, conf, occ))
    mx = lambda e, m: float(e[m].max()) if bool(m.any()) else 0.0
    well = ref.conf >= CONF_WELL
    ed = (disp - ref.disp).abs()
    return Errors(not_sure=float((~ref.sure).double().mean()), sure_mismatch=int((~same & ref.sure).sum()),
                  planted_mismatch=int((~same & planted).sum()), agree=float(same.double().mean()),
                  conf=mx((conf - ref.conf).abs(), same), disp=mx(ed, same & well), disp_low=mx(ed, same & ~well),
                  occ=float((occ - ref.occ).abs().max()), occ_min=float(occ.min()), occ_max=float(occ.max()), finite=finite)


@functools.lru_cache(maxsize=None)
def yardstick(w, pos, dtype, h=2, B=1, ot_iter=3):
    """the fp32 oracle's own distance from the float64 reference on a case"""
    return compare(build(w, pos, dtype, h, B), reference(w, pos, dtype, h, B, ot_iter), *oracle_fp32(w, pos, dtype, h, B, ot_iter))


def tol_disp_low(w, yard):
    """disp = i - (num + 1e-4) / (conf + 1e-4), num about argmax * conf: once conf is comparable to 1e-4 the two no longer cancel and a
    relative error r of the window's probabilities moves disp by up to argmax * r * 1e-4 * conf / (conf + 1e-4)^2 <= argmax * r / 4 --
    4e-3 at argmax = 1500, r = 1e-5, against 5e-6 where conf is large.  Only token-like volumes have such pixels (every occluded one).
    From conf = CONF_WELL up the factor is below argmax * 1e-4 / conf = 15 at w = 1536: 1.5e-4 for r = 1e-5, inside tol_disp, which
    holds there unchanged.  Below it the bound is the fp32 oracle's own distance from float64 on the same pixels of the same case times
    MARGIN = 3: K2 works in the log2 domain (potentials 1.44 times larger, so their fp32 rounding is 1.4 times coarser in natural units) and
    the maximum of a few dozen such pixels of two independent roundings differs by a factor of about two.  Never below tol_disp."""
    return max(tol_disp(w), MARGIN * yard.disp_low)


def check(case, e, yard):
    """the asserts of item 4 on the Errors of one run; the list of the ones that fail (empty: the run passes)"""
    w, bad = case.w, []
    if not e.finite:
        bad.append("an output is not finite")
    if e.not_sure > NOT_SURE_CAP:
        bad.append(f"{100 * e.not_sure:.2f} % of the pixels are not sure (cap {100 * NOT_SURE_CAP:.0f} %)")
    if e.sure_mismatch:
        bad.append(f"{e.sure_mismatch} argmax mismatches on sure pixels")
    if e.planted_mismatch:
        bad.append(f"{e.planted_mismatch} argmax mismatches on planted pixels")
    if not e.conf < TOL_CONF:
        bad.append(f"conf {e.conf:.3g} >= {TOL_CONF:.3g}")
    if not e.occ < TOL_OCC:
        bad.append(f"occ {e.occ:.3g} >= {TOL_OCC:.3g}")
    if not e.disp < tol_disp(w):
        bad.append(f"disp (conf >= {CONF_WELL}) {e.disp:.3g} >= {tol_disp(w):.3g}")
    if not e.disp_low < tol_disp_low(w, yard):
        bad.append(f"disp (conf < {CONF_WELL}) {e.disp_low:.3g} >= {tol_disp_low(w, yard):.3g} (fp32 oracle {yard.disp_low:.3g})")
    if not (e.occ_min >= 0 and e.occ_max <= 1 + 1e-5):
        bad.append(f"occ in [{e.occ_min:.3g}, {e.occ_max:.8g}], not in [0, 1 + 1e-5]")
    return bad


def line(case, ot_iter, e, yard, note="", switch_on=True):
    form = "TRI" if uses_tri(case.w, case.dtype, case.pos, switch_on) else "   "
    return (f"w {case.w:4d} B{case.B} h{case.h} {SHORT[case.dtype]} pos {int(case.pos)} ot_iter {ot_iter} {lanes(case.w)}x{chunks(case.w)} {form}"
            f"  not sure {100 * e.not_sure:4.2f} %  agree {e.agree:.4f}  conf {e.conf:.2e} ({yard.conf:.2e})  occ {e.occ:.2e} ({yard.occ:.2e})"
            f"  disp {e.disp:.2e} ({yard.disp:.2e}) / {tol_disp(case.w):.2e}  low conf {e.disp_low:.2e} ({yard.disp_low:.2e}) / "
            f"{tol_disp_low(case.w, yard):.2e}{note}")
