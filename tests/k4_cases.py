"""Cases, inputs, the float64 reference, the elementwise bounds, the one comparator and a torch emulation (with deliberately wrong variants) of
K4 (s2m2_attention, csrc/attention.hip), shared by tests/test_hip_k4_plans.py (the kernel through the C ABI) and tests/test_k4_cases_cpu.py
(every claimed plan asked of the planner through s2m2_attention_plan, coverage of the planner's branches, the emulation and its wrong
variants through this comparator): what rejects a wrong variant on the CPU is literally what the GPU test runs.

A case is (nb, heads, Nq, Nk, D), a dtype, swap_halves, an optional token grid (PE variant) and the launch plan it claims (k4_plans.PLANS,
literal).  tests/test_k4_cases_cpu.py compares every claim with the planner, so a moved threshold in launch_attn fails there and cannot
quietly put these cases onto another plan.

Inputs (inputs()): one row buffer of width 3 * heads * D holding [q | k | v] per token row, as the fused projection of the forward does, with
GUARD rows of large finite values before and after.  Nq == Nk: q, k, v are channel slices of the same rows; otherwise the nb * Nq query rows
are followed by the nb * Nk key / value rows.  Values are drawn in fp32 and rounded to the case's dtype; reference and emulation read the
rounded values.  Per query i:
  i % 3 == 0  flat row: q = 0.5 randn against k = 0.5 randn
  i % 3 == 1  peaked row: q is PEAK / (scale |k_j|^2) * k_j for a key j taken in turn from peak_keys(): key Nk - 1, key 0, the first key of
              the last stage, the last key of the first stage, a key in each wave's share (sub-tile w of four) of the first and of the
              last stage -- with the stage length of the claimed plan
  i % 3 == 2  common row: every key carries BETA in channel 0, these queries -COMMON / (BETA scale): every true score is about -COMMON, a
              phantom key of score 0 dominates the row
Key 0 of every batch is a magnet: its key 4 times larger, its value 3 + a ramp over the channels + batch + head.  A bound that runs one
row past Nk reads the magnet of the next batch, or the guard row (k = 8, v = 50) behind the last one.  The largest |score * scale| is about
PEAK + a few units for the peaked rows and COMMON for the common rows: nothing leaves the range of fp16 or of exp.

Reference (reference()): float64 softmax(Q K^T scale) V with the fp32 value of scale the launch receives, on the device the inputs live on,
in chunks of batches / queries; for PE cases also pe_sum[q] = sum_k a_k * 0.5 * [px[xq - xk + w - 1], py[yq - yk + h - 1]], the einsum
'nij,ijc->nic' of the reference model's attentions.py:47, in float64.

Bounds, elementwise, from the arithmetic and nothing measured.  For one query: t_k = score_k * scale (natural-log units), a_k the float64
softmax weights, ref = sum_k a_k v_k, S_k = sum_d |q_d k_d|, tmax = max_k t_k.  The kernel computes p_k = exp2(fma(s_k, scale2, -m)) with s_k
accumulated in fp32 by the MFMAs, a row sum L = sum p_k in fp32, N = sum p_k v_k on the MFMAs with fp32 accumulators (p_k rounded to fp16 first
in fp16 mode), out = N / L.  Any common factor of all p_k -- the running maximum, the rescales alpha of the online form, the merge factors
of the key-split form, all applied to N and L alike -- cancels except for its roundings.  So out = sum a_k (1 + e_k) (1 + h_k) (1 + g) v_k /
sum a_k (1 + e_k) (1 + g') with
  e_k   relative error of p_k:   scale * D * U24 * S_k        fp32 accumulation of the score (D terms, any order)
                               + T_ROUNDINGS * U24 * (tmax - t_k)   the fma's rounding and the two roundings in scale * log2(e)
                               + EXP2_REL                     v_exp_f32
  h_k   P rounded to fp16 (fp16 only): U11, and an absolute 2^-25 below the normal range -- relative to L >= 1: Nk * 2^-25 * max_k |v_k|
  g, g' fp32 accumulation of N and L, (Nk + TAIL_OPS) * U24: Nk additions in any order, the rescales (at most Nk / 32 of them), the merge of four
        partial states, 1 / L and the last product; pe_sum: also the contraction of the max(w, h) marginal bins with the table rows
With dN = sum a_k |v_k| ((1 + e_k)(1 + h)(1 + g) - 1) [+ the subnormal term] and dL = sum a_k ((1 + e_k)(1 + g') - 1), exactly
  |out - ref| <= (dN + |ref| dL) / (1 - dL),
and the fp16 output adds its rounding U11 * (|ref| + that) + 2^-25.  pe_sum: the same with the 0.5-weighted table rows in place of v.
(Weights below 2^-126 of the largest flush to zero in the kernel: sum of at most Nk * 2^-126 * max|v|, below every term above.)
"""
import collections
import functools

import torch

import k4_plans

TDT = {"float32": torch.float32, "float16": torch.float16}
SHORT = {"float32": "fp32", "float16": "fp16"}
U24, U11 = 2.0 ** -24, 2.0 ** -11
T_ROUNDINGS = 3          # roundings that scale with |t_k - tmax|: scale * log2(e) (constant rounded to fp32, product rounded), the fma's result
EXP2_REL = 2 * U24       # v_exp_f32: 1 ulp (CDNA ISA guide, transcendental accuracy)
TAIL_OPS = 16            # roundings on N and L beside the Nk additions: 4 merge products + 3 additions, 1 / L, the final product, 0.5 (pe_sum); rest spare
GUARD = 2                # rows before and after the tokens
GUARD_QK, GUARD_V = 8.0, 50.0
BETA, COMMON, PEAK = 2.0, 10.0, 8.0
PLAN_FIELDS = k4_plans.FIELDS

Plan = collections.namedtuple("Plan", PLAN_FIELDS)


class Case(collections.namedtuple("Case", "nb heads Nq Nk D dt swap grid plan")):
    @property
    def id(self):
        g = f"-pe{self.grid[0]}x{self.grid[1]}" if self.grid else ""
        return f"{self.nb}x{self.heads}x{self.Nq}x{self.Nk}x{self.D}{'-swap' if self.swap else ''}{g}-{SHORT[self.dt]}"

    @property
    def shape(self):
        return (self.nb, self.heads, self.Nq, self.Nk, self.D)

    @property
    def C(self):
        return self.heads * self.D

    @property
    def stage(self):
        """keys per stage of the claimed plan"""
        return 32 * self.plan.kt

    @property
    def nstage(self):
        return -(-self.Nk // self.stage)

    @property
    def scale(self):
        """the fp32 value the launch receives"""
        return float(torch.tensor(self.D ** -0.5, dtype=torch.float32))

    def small(self):
        """the case the CPU tests run the emulation on: (Nq, Nk, D), dtype, swap, grid and plan kept, nb and heads cut to 2 (4 batches
        where swap_halves is set: with two, (b + 1) % nb is (b + nb / 2) % nb)"""
        nb = min(self.nb, 4 if self.swap else 2)
        return self._replace(nb=nb, heads=min(self.heads, 2))


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    for (nb, heads, Nq, Nk, D, swap, grid), by_dt in k4_plans.PLANS.items():
        for dt, p in by_dt.items():
            out.append(Case(nb, heads, Nq, Nk, D, dt, swap, grid, Plan(*p)))
    return tuple(out)


def bkv(case, b):
    return (b + case.nb // 2) % case.nb if case.swap else b


def peak_keys(case):
    Nk, st = case.Nk, case.stage
    last0 = (case.nstage - 1) * st
    ks = [Nk - 1, 0, last0, st - 1]
    ks += [w * 32 + 5 for w in (1, 2, 3)] + [last0 + w * 32 + 5 for w in (1, 2, 3)]
    if case.plan.kt == 8:
        ks += [w * 32 + 5 for w in (5, 6)]
    seen = []
    for k in ks:
        if 0 <= k < Nk and k not in seen:
            seen.append(k)
    return seen


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
class Inputs(collections.namedtuple("Inputs", "buf q k v q_row0 kv_row0 px py")):
    """buf (rows, 3C) with the guard rows; q (nb, Nq, C), k, v (nb, Nk, C) views into it; px, py fp32 tables (PE cases)"""


def _fill(case):
    nb, heads, Nq, Nk, D = case.shape
    g = torch.Generator().manual_seed(((nb * 131 + heads) * 8209 + Nq) * 8209 + Nk * 389 + D + (case.dt == "float16") * 7 + case.swap * 13)
    rn = lambda *s: torch.randn(*s, generator=g)
    q, k, v = 0.5 * rn(nb, Nq, heads, D), 0.5 * rn(nb, Nk, heads, D), rn(nb, Nk, heads, D)
    k[:, 0] *= 4.0                                                                    # the magnet
    k[..., 0] = BETA
    ramp = 0.25 * (torch.arange(D) % 16).float()
    v[:, 0] = 3.0 + ramp[None, None, :] + torch.arange(nb).float()[:, None, None] + torch.arange(heads).float()[None, :, None]
    scale = case.scale
    pk = peak_keys(case)
    kb = torch.stack([k[bkv(case, b)] for b in range(nb)])                            # the keys batch b attends to
    i1 = torch.arange(1, Nq, 3)
    if i1.numel():
        j = torch.tensor([pk[(int(i) // 3) % len(pk)] for i in i1])
        kj = kb[:, j]                                                                 # (nb, n, heads, D)
        q[:, i1] = PEAK / (scale * (kj * kj).sum(-1, keepdim=True)) * kj
    q[:, 2::3, :, 0] = -COMMON / (BETA * scale)
    return q, k, v


@functools.lru_cache(maxsize=2)
def inputs(case, device="cpu"):
    """built once and shared; nothing may write into them"""
    nb, heads, Nq, Nk, D = case.shape
    C = case.C
    q, k, v = _fill(case)
    shared = Nq == Nk
    nrow = GUARD + nb * Nq + (0 if shared else nb * Nk) + GUARD
    buf = torch.empty(nrow, 3 * C)
    buf[:, :2 * C] = GUARD_QK
    buf[:, 2 * C:] = GUARD_V
    q0 = GUARD
    kv0 = GUARD if shared else GUARD + nb * Nq
    buf[q0:q0 + nb * Nq, :C] = q.reshape(nb * Nq, C)
    buf[kv0:kv0 + nb * Nk, C:2 * C] = k.reshape(nb * Nk, C)
    buf[kv0:kv0 + nb * Nk, 2 * C:] = v.reshape(nb * Nk, C)
    buf = buf.to(TDT[case.dt]).to(device)
    qv = buf[q0:q0 + nb * Nq].view(nb, Nq, 3 * C)[..., :C]
    kr = buf[kv0:kv0 + nb * Nk].view(nb, Nk, 3 * C)
    px = py = None
    if case.grid:
        from s2m2_amd.engine import pe_tables
        px, py = pe_tables(case.grid[1], case.grid[0], "cpu")
        px, py = px.to(device), py.to(device)
    return Inputs(buf, qv, kr[..., C:2 * C], kr[..., 2 * C:], q0, kv0, px, py)


def heads_of(t, heads):
    """(nb, N, heads * D) -> (nb, heads, N, D)"""
    return t.reshape(t.shape[0], t.shape[1], heads, -1).transpose(1, 2)


def grid_xy(case, device):
    gw, gh = case.grid
    i = torch.arange(gw * gh, device=device)
    return i % gw, i // gw


# ---- reference and bounds -----------------------------------------------------------------------------------------------------------------
Ref = collections.namedtuple("Ref", "out bound pe pe_bound")        # (nb, Nq, C) float64 each; pe, pe_bound (nb, Nq, heads * 32) or None
CHUNK = 1 << 22                                                      # score elements per chunk of the float64 evaluation


def _chunks(case):
    nb, heads, Nq, Nk, _ = case.shape
    per_b = heads * Nq * Nk
    if per_b <= CHUNK:
        nbc = max(1, CHUNK // per_b)
        return [(slice(b, min(b + nbc, nb)), slice(0, Nq)) for b in range(0, nb, nbc)]
    qc = max(1, CHUNK // (heads * Nk))
    return [(slice(b, b + 1), slice(i, min(i + qc, Nq))) for b in range(nb) for i in range(0, Nq, qc)]


def weights64(q, k, scale):
    """float64 softmax weights and the per-key relative error bound e_k of the kernel's p_k (module docstring)"""
    D = q.shape[-1]
    t = torch.matmul(q, k.transpose(-1, -2)) * scale
    S = torch.matmul(q.abs(), k.abs().transpose(-1, -2))
    tmax = t.max(-1, keepdim=True).values
    a = torch.softmax(t, -1)
    e = scale * D * U24 * S + T_ROUNDINGS * U24 * (tmax - t) + EXP2_REL
    return a, e


def bound_terms(a, e, vals, ref, Nk, fp16, extra_ops=0):
    """vals (.., Nk, c): what the weights are contracted with (V, or the 0.5-weighted table rows of pe_sum: then (.., Nq, Nk, c))"""
    g = (Nk + TAIL_OPS + extra_ops) * U24
    wn = a * ((1 + e) * (1 + (U11 if fp16 else 0.0)) * (1 + g) - 1)
    wl = a * ((1 + e) * (1 + g) - 1)
    va = vals.abs()
    if va.dim() == a.dim():
        dN = torch.matmul(wn, va)
        vmax = va.max(-2, keepdim=True).values
    else:
        dN = torch.einsum("...ij,...ijc->...ic", wn, va)
        vmax = va.max(-2).values
    if fp16:
        dN = dN + Nk * 2.0 ** -25 * vmax
    dL = wl.sum(-1, keepdim=True)
    b = (dN + ref.abs() * dL) / (1 - dL)
    if fp16:
        b = b + U11 * (ref.abs() + b) + 2.0 ** -25
    return b


@functools.lru_cache(maxsize=2)
def reference(case, device="cpu"):
    inp = inputs(case, device)
    nb, heads, Nq, Nk, D = case.shape
    fp16 = case.dt == "float16"
    f64 = dict(dtype=torch.float64, device=device)
    out, bnd = torch.empty(nb, heads, Nq, D, **f64), torch.empty(nb, heads, Nq, D, **f64)
    pe = pb = None
    if case.grid:
        gw, gh = case.grid
        xs, ys = grid_xy(case, device)
        pe, pb = torch.empty(nb, heads, Nq, 32, **f64), torch.empty(nb, heads, Nq, 32, **f64)
    kvb = torch.tensor([bkv(case, b) for b in range(nb)], device=device)
    for bs, qs in _chunks(case):
        q = heads_of(inp.q[bs, qs].double(), heads)
        k = heads_of(inp.k[kvb[bs]].double(), heads)
        v = heads_of(inp.v[kvb[bs]].double(), heads)
        a, e = weights64(q, k, case.scale)
        r = torch.matmul(a, v)
        out[bs, :, qs] = r
        bnd[bs, :, qs] = bound_terms(a, e, v, r, Nk, fp16)
        if case.grid:
            step = max(1, (1 << 21) // Nk)                                               # the dense (q, k, 32) encoding, a few queries at a time
            for i0 in range(qs.start, qs.stop, step):
                sl = slice(i0, min(i0 + step, qs.stop))
                tab = 0.5 * torch.cat([inp.px.double()[xs[sl, None] - xs[None, :] + gw - 1], inp.py.double()[ys[sl, None] - ys[None, :] + gh - 1]], 2)
                al, el = a[:, :, sl.start - qs.start:sl.stop - qs.start], e[:, :, sl.start - qs.start:sl.stop - qs.start]
                rp = torch.einsum("bhij,ijc->bhic", al, tab)
                pe[bs, :, sl] = rp
                pb[bs, :, sl] = bound_terms(al, el, tab, rp, Nk, fp16, extra_ops=max(gw, gh))
    tok = lambda t: t.transpose(1, 2).reshape(nb, Nq, -1)
    return Ref(tok(out), tok(bnd), tok(pe) if pe is not None else None, tok(pb) if pb is not None else None)


# ---- comparator ---------------------------------------------------------------------------------------------------------------------------
Result = collections.namedtuple("Result", "err bound ratio nbad n where")


def compare(out, ref, bound):
    """every element of out against ref under bound: the element of the worst error / bound.  An element that is not finite (the NaN
    prefill of a buffer: never written) has ratio inf."""
    o = out.detach().double()
    assert o.shape == ref.shape == bound.shape, (o.shape, ref.shape, bound.shape)
    err = (o - ref).abs()
    ratio = torch.where(torch.isfinite(err), err / bound, torch.full_like(err, float("inf")))
    k = int(ratio.argmax())
    return Result(float(err.flatten()[k]), float(bound.flatten()[k]), float(ratio.flatten()[k]), int((ratio > 1).sum()), ratio.numel(),
                  tuple(int(i) for i in torch.unravel_index(torch.tensor(k), ratio.shape)))


def line(case, res, what="out", note=""):
    p = case.plan
    plan = (f"DP{p.dp:3d} MINW{p.minw} {'ksplit' if p.ksplit else '      '} {p.nw}w x {p.nblk:3d}blk KT{p.kt}{' 2pass' if p.twopass else ''}{' qlds' if p.qlds else ''}"
            f"{' deep' if p.deep else ''}{f' bins{p.nxt}x{p.nyt}' if p.nxt else ''} lds{p.lds}")
    return (f"{case.id:38s} {plan:58s} {what:3s} max err {res.err:.3e}  bound {res.bound:.3e}  ratio {res.ratio:.3f}  over 1: {res.nbad} of {res.n}"
            f"  at {res.where}  {'ok' if res.ratio <= 1 else 'FAIL'}{note}")


# ---- emulation of the kernel's arithmetic, and wrong variants of it -------------------------------------------------------------------------
VARIANTS = ("drop_last_key", "zero_key", "next_row_key", "subtile_twice", "skip_stage", "no_rescale", "merge_drops_wave", "scale_dp",
            "head_offset_dp", "swap_ignored", "swap_plus_one", "pe_row_off_by_one", "pe_tables_exchanged")


def dp_of(case):
    return (case.D + 15) // 16 * 16


def applies(variant, case):
    """does the case have the feature the variant breaks?"""
    p = case.plan
    return {
        "drop_last_key": True, "zero_key": True, "next_row_key": True,
        "subtile_twice": case.Nk > 32, "skip_stage": case.nstage > 1,
        "no_rescale": case.Nk > 32 and not p.twopass,                 # the two-sweep form has no rescale
        "merge_drops_wave": bool(p.ksplit),
        "scale_dp": dp_of(case) != case.D, "head_offset_dp": dp_of(case) != case.D and case.heads > 1,
        "swap_ignored": bool(case.swap), "swap_plus_one": bool(case.swap),
        "pe_row_off_by_one": case.grid is not None and case.grid[1] > 1, "pe_tables_exchanged": case.grid is not None,
    }[variant]


def exempt(variant, case):
    """a case the variant's feature applies to but the variant cannot change: the rule, or None"""
    if variant == "swap_plus_one" and case.nb == 2:
        return "two batches: (b + 1) % nb is (b + nb / 2) % nb"
    return None


def _gather(inp, rows, col0, hstride, heads, D):
    """(nb, heads, N, D) fp32 read from the row buffer as the kernel addresses it: element (row, col0 + hd * hstride + e)"""
    W = inp.buf.shape[1]
    cols = col0 + (torch.arange(heads, device=rows.device) * hstride)[:, None] + torch.arange(D, device=rows.device)[None, :]
    idx = rows[:, None, :, None] * W + cols[None, :, None, :]
    return inp.buf.flatten()[idx].float()


def emulate(case, variant=None, device="cpu"):
    """K4's arithmetic in torch: operands in the I/O dtype, fp32 scores, softmax against the exact row maximum, P rounded to fp16 for the PV
    product in fp16 mode (the row sum takes the unrounded p), fp32 accumulation, the output rounded to the I/O dtype.  -> out [, pe_sum]"""
    inp = inputs(case, device)
    nb, heads, Nq, Nk, D = case.shape
    C, st = case.C, case.stage
    fp16 = case.dt == "float16"
    hstride = dp_of(case) if variant == "head_offset_dp" else D
    scale = float(torch.tensor(dp_of(case) ** -0.5, dtype=torch.float32)) if variant == "scale_dp" else case.scale
    kvb = [bkv(case, b) for b in range(nb)]
    if variant == "swap_ignored":
        kvb = list(range(nb))
    if variant == "swap_plus_one":
        kvb = [(b + 1) % nb for b in range(nb)]
    kidx = torch.arange(Nk)
    if variant == "drop_last_key":
        kidx = kidx[:-1]
    if variant == "next_row_key":
        kidx = torch.arange(Nk + 1)                                  # row Nk: the next batch's first row, or the guard row
    if variant == "subtile_twice":                                    # the last 32-key sub-tile is read from where the first one lies
        s1 = (Nk - 1) // 32 * 32
        kidx = torch.where(kidx >= s1, kidx - s1, kidx)
    if variant == "skip_stage":
        kidx = kidx[kidx < (case.nstage - 1) * st]                    # the last stage
    if variant == "merge_drops_wave":
        kidx = kidx[(kidx % st) // 32 % 4 != 1]                       # wave 1's sub-tiles of every stage
    tile = torch.arange(kidx.numel()) // 32
    if variant == "zero_key":
        tile = torch.cat([tile, tile[-1:]])
    qrows = inp.q_row0 + torch.arange(nb)[:, None] * Nq + torch.arange(Nq)[None, :]
    krows = inp.kv_row0 + torch.tensor(kvb)[:, None] * Nk + kidx[None, :]
    q = _gather(inp, qrows.to(device), 0, hstride, heads, D)
    k = _gather(inp, krows.to(device), C, hstride, heads, D)
    v = _gather(inp, krows.to(device), 2 * C, hstride, heads, D)
    if variant == "zero_key":
        k = torch.cat([k, torch.zeros_like(k[:, :, :1])], 2)
        v = torch.cat([v, torch.zeros_like(v[:, :, :1])], 2)
    out = torch.full((nb, heads, Nq, D), float("nan"), device=device)
    pe = torch.full((nb, heads, Nq, 32), float("nan"), device=device) if case.grid else None
    nq_run = Nq if k.shape[2] else 0                                  # no key left: 0 / 0 everywhere
    if case.grid:
        gw, gh = case.grid
        xs, ys = grid_xy(case, device)
        kx, ky = kidx.to(device) % gw, kidx.to(device) // gw          # (a key past the grid falls into no y bin)
        if variant == "zero_key":
            kx, ky = torch.cat([kx, kx.new_tensor([-1])]), torch.cat([ky, ky.new_tensor([-1])])
        if variant == "pe_row_off_by_one":                            # floor(kv / gw) one short where kv is a multiple of gw: x = gw has no bin
            hit = (kx == 0) & (ky > 0)
            ky[hit] -= 1
            kx[hit] = gw
        ohx = (kx[:, None] == torch.arange(gw, device=device)[None, :]).float()
        ohy = (ky[:, None] == torch.arange(gh, device=device)[None, :]).float()
        tx = inp.px[xs[:, None] - torch.arange(gw, device=device)[None, :] + gw - 1]      # (Nq, gw, 16)
        ty = inp.py[ys[:, None] - torch.arange(gh, device=device)[None, :] + gh - 1]
    qc = max(1, (1 << 23) // (nb * heads * max(1, k.shape[2])))
    for i0 in range(0, nq_run, qc):
        sl = slice(i0, min(i0 + qc, Nq))
        t = torch.matmul(q[:, :, sl], k.transpose(-1, -2)) * scale
        m = t.max(-1, keepdim=True).values
        p = torch.exp(t - m)
        l = p.sum(-1, keepdim=True)
        if variant == "no_rescale":                                   # O keeps every sub-tile's p relative to the running maximum of its time
            nt = int(tile.max()) + 1
            tm = torch.full(t.shape[:-1] + (nt,), -float("inf"), device=device)
            tm = tm.scatter_reduce(-1, tile.to(device).expand(t.shape), t, "amax")
            run = torch.cummax(tm, -1).values
            p = torch.exp(t - run.gather(-1, tile.to(device).expand(t.shape)))
        if fp16:
            p = p.half().float()
        out[:, :, sl] = torch.matmul(p, v) / l
        if case.grid:
            mx, my = torch.matmul(p, ohx) / l, torch.matmul(p, ohy) / l
            ex = 0.5 * torch.einsum("bhix,ixc->bhic", mx, tx[sl])
            ey = 0.5 * torch.einsum("bhiy,iyc->bhic", my, ty[sl])
            pe[:, :, sl] = torch.cat([ey, ex] if variant == "pe_tables_exchanged" else [ex, ey], -1)
    tok = lambda x: x.transpose(1, 2).reshape(nb, Nq, -1).to(TDT[case.dt])
    return (tok(out), tok(pe)) if case.grid else tok(out)
