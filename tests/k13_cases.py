"""Cases, plain operands, inputs, the float64 reference, a float64 emulation of the kernel's rounding points (with deliberately wrong variants),
the bounds and the one comparator of K13 (s2m2_row_attn, csrc/rowattn.hip), shared by tests/test_hip_k13_rows.py (the kernel through the raw C
entry) and tests/test_k13_cases_cpu.py (coverage of the wave counts, chunks and counted waits computed as the kernel computes them, the
emulation through this comparator, the leave-one-out check of the bound and the rejection of every wrong variant): what rejects a wrong
variant on the CPU is literally what the GPU test runs.

Operands      A case is built from PLAIN (128, 128) fp16 layers q, k, v, proj, ffn.0, ffn.2 and plain fp32 vectors (operands()).  The reference
              model's pre-LayerNorms have no affine (attentions.py:117,148,243: elementwise_affine=False) and its q, k and proj no bias, so the
              engine's row_step (engine.py:556-570) packs zero rows 0, 2 and 6 of the vector block.  The kernel's entry takes all twelve rows,
              and a checkpoint whose pre-LN carries an affine folds it exactly as fold() does: W' = fp16(W * gamma), b' = b + W . beta, row
              sums of W'.  The `full` regime folds non-trivial (gamma, beta) pairs, which makes the q and k biases non-zero, and gives proj a
              bias of its own: all six biases and both ln_out vectors are non-zero.  fold() with no affine is the engine's packing, and
              tests/test_k13_cases_cpu.py asserts that equality on a BasicAttnBlock of seeded_state_dict.  The reference never sees a packed
              tensor; the kernel gets pack.rowattn_pack / pack.rowattn_vectors of the same plain operands (packed()).
Inputs        x is the channel slice [pad, pad + 128) of rows 1 .. n of an (n + 2, x_stride) buffer whose every other element is GUARD_X
              (200): a read outside the tokens changes a result and stays inside the allocation.
Reference     reference(): the step in float64 on the fp16 inputs with no intermediate rounding:  z' = z + proj(attn(LN z, LN s)),
              out = z' + ffn(LN z'), ln = LayerNorm(out) gamma + beta; s = the same line of image (n + nimg / 2) % nimg (cross) or z.
Emulation     emulate(): float64 arithmetic that rounds to fp16 at exactly the ten points the header of rowattn.hip names -- Q, K, V, the
              probabilities, the attention output, the proj output, the residual sum, the FFN hidden tensor, the FFN output, the final sum --
              with the kernel's per-32-key online softmax in the log2 domain (the probabilities are rounded against the RUNNING maximum, the
              row sum takes them unrounded), the LN fold rstd * (acc - mean * wsum) + bias with the one-pass variance q / C - mean^2 clamped
              at 0, its sums taken in fp32 in the order a half-wave takes them (ln_stats()), and the two-pass ln_out of the stored rows.
              flips=seed moves every rounded intermediate that is not zero to a neighbouring fp16 value, with probability 1/8 up and 1/8 down:
              the fp32 summation order of the MFMAs, v_exp_f32 and the fast GELU (tests/test_gelu16_cpu.py: within one ulp of the correctly
              rounded value) decide the last bit one way or the other.  The two residual sums are NOT flipped: each adds two fp16 values,
              which is exact in fp32, and from_f32 rounds that correctly -- none of the three sources can move them (flipping them as well
              widens D_t and lets an ensemble member with two flips on one large channel fail the leave-one-out check).

Regimes
  full        Gaussian layers of the model's scale (N(0, 1 / C)).  Token t of a row has offset OFFS[(t + 2 line) % 3] and scale
              SCALES[(t + line) % 2], so neighbours inside one 32-token tile differ in both; token w / 2 of row 0 is the constant 1.5
              (variance exactly 0: rstd = eps^-1/2); in `hot` cases token 1 of the last row is the constant HOT, an 11-bit value whose sum of
              squares rounds in fp32 so that the one-pass variance comes out NEGATIVE in the order ln_stats() sums (the clamp decides between
              rstd = eps^-1/2 and NaN).  Every tenth query (t % 10 == 3) is aimed at key w - 1 of its source row: its normalised direction
              is 0.8 of the standardised gradient of that logit.
              Measured on the S model's forward (CPU oracle, synthetic_pair 128 x 192 and 256 x 320, seeded weights): the tokens that enter
              and leave the 1-D attention blocks at the 1/4 and 1/8 levels, feature_tr_4x included, have |mean| / std of at most TOKEN_RATIO
              (see its comment).  OFFS / SCALES reach 4 / 0.25 = 16.
              Judged per token, no element and no token exempt: D_t = the largest |E_s - R| over the 128 channels of token t and over the
              round-to-nearest emulation and eight flipped ones; every element of token t must be within ulp16(max(1, |R|)) + 2 D_t of R.
              The factor 2 is taken over the reference's own rounding noise because nine draws under-sample its maximum; the CPU tests show
              it neither too tight (leave-one-out: every member passes the bound built from the other eight) nor too loose (every wrong
              variant fails it).
  route       proj is the exact identity without bias and ffn.2 is zero, so out = fp16(o + x).  A head's channels are [c, -c, k, -k]: a query
              code and a key code, each a +-1 codeword of the Reed-Muller code RM(2, m) next to its negation (mean exactly 0, variance exactly
              amplitude^2; two different codewords agree in at most 3/4 of their positions), times an amplitude of ROUTE_AMPS that the
              LayerNorm removes.  q = A LN(x)[c, -c], k = A LN(s)[k, -k], v = LN(s) + bv.  Query i carries the key code of key pi_h(i) of its
              source row: that key's logit exceeds every other by more than 40 in the log2 domain (asserted on the CPU), the probabilities
              are 0 or 1 after rounding and out names the key each query took.  i % 4 == 0: a key of the LAST tile (the running maximum rises
              in the last tile visited); i % 4 == 1: key 0, key w - 1, the first and last key of every 32-tile and both sides of the 160-key
              chunk boundary in turn; the rest: a seeded permutation.  Bound: route_bound(), from the arithmetic alone (half an ulp of v, half
              an ulp of the sum, the LN term): a flipped emulation does not pass it, only the round-to-nearest one is held to it.
  probes      identity and zero layers make one stage visible, so an analytic elementwise bound stays useful (through one or two 128-wide
              layers worst-case propagation is; through six it is not).  On the full regime's tokens:
              attn    proj the exact identity, ffn.2 zero: out = fp16(o + x); attn_probe_bound(): K4's bound (k4_cases.weights64,
                      bound_terms) with the q, k, v errors of ln_fold_bound() carried into the weights;
              ffn     proj zero: z' = x exactly; ffn_probe_bound(): the LN fold, GELU (k5_cases.GELU_ABS, one fp16 ulp), ffn.2, two sums;
              pass    proj and ffn.2 zero: out must equal x bit for bit and ln_out is the two-pass LayerNorm of it (ln_out_bound()); tokens
                      64 + k / 16, k in 0 .. 6 -- |mean| / std of 500, where a one-pass variance in fp32 loses the variance.
              and on the route regime's tokens:
              tail    the V layer is zero with a bias c, so o = c whichever key is taken; proj is twice a rotation of the channels plus a
                      non-zero bias; c, the bias and the tokens are sixteenths, so z' = x + proj(o) is an fp16 value the kernel owes exactly
                      and ffn_probe_bound() applies behind it: proj, its bias (vector row 6) and the first residual sum under an analytic
                      bound, two layers deep.
              If a correct kernel exceeds an analytic bound, a rounding is missing from its derivation: find it and write it down.

Wrong kernels VARIANTS, each expressed in emulate(); applies() says which cases have the feature a variant breaks, exempt() which of those
              cannot show it.
"""
import collections
import functools
import math

import numpy as np
import torch

from s2m2_amd import pack

C = 128
EPS = 1e-5
LN_OUT_EPS = 1e-5
GUARD_X = 200.0
OFFS = (0.0, 1.0, 4.0)
SCALES = (0.25, 1.5)
HOT = 8.0078125                                  # 1025 / 128: eleven significant bits
# largest |mean| / std of a token entering or leaving a 1-D attention block of the S forward (1/4 and 1/8 levels, feature_tr_4x included),
# CPU oracle (oracle.s2m2_oracle.forward with basic_attn_block wrapped to record its input and output; tests/test_k13_cases_cpu.py repeats the
# measurement at 128 x 192), synthetic_pair(128, 192) and (256, 320), seeded weights: 0.32 at the input of enc_attn0 (1/4 level), 0.19 at the 1/8 level, 0.18
# in feature_tr_4x (token std 0.4 .. 4.5, |mean| <= 0.65); the stress range 4 / 0.25 = 16 is far above twice that
TOKEN_RATIO = 0.33
FLIP_SEEDS = tuple(range(1, 9))
LOG2E = float(np.float32(1.44269504088896340736))
WIDTHS = (8, 31, 32, 33, 96, 128, 159, 160, 161, 192, 224, 225, 257, 288, 319, 320)
X_STRIDES, OUT_STRIDES, LN_STRIDE = (128, 136, 260), (128, 132), 140
PROBES = ("attn", "ffn", "pass", "tail")         # the probe regimes
ROUTED = ("route", "tail")                       # regimes on the route tokens (every query has a magnet key)
ROUTE_A = {1: 4.0, 2: 5.0}                       # the gain of the route regime's q and k layers, per head count
TAIL_SHIFT = 37                                  # the tail probe's proj: output channel i = 2 x input channel (i + 37) % 128 + bias
ROUTE_AMPS = (0.5, 1.0, 2.0)                     # token amplitudes of the route regime (the LayerNorm removes them; the statistics differ)


class Case(collections.namedtuple("Case", "w heads cross nimg h regime ln_out xs os ls xcd hot")):
    @property
    def id(self):
        s = f"w{self.w}-H{self.heads}-{'x' if self.cross else 's'}-n{self.nimg}h{self.h}-{self.regime}"
        s += "-ln" if self.ln_out else ""
        s += f"-xs{self.xs}-os{self.os}" + ("" if self.xcd else "-noxcd") + ("-hot" if self.hot else "")
        return s

    @property
    def rows(self):
        return self.nimg * self.h

    # ---- what the kernel derives from w (csrc/rowattn.hip) ----
    @property
    def nwv(self):
        return (self.w + 31) // 32

    @property
    def ntile(self):
        return (self.w + 31) >> 5

    @property
    def nchunk(self):
        return (self.ntile + 4) // 5

    @property
    def threads(self):
        """the instantiation's launch bound"""
        return 320 if self.nwv <= 5 else 640

    def nkv(self, wv):
        """LDS-DMA instructions wave wv issues for Wk and Wv"""
        return 2 * ((32 - wv + self.nwv - 1) // self.nwv)

    def entry_wait(self, wv):
        """the vmcnt the entry phase waits for"""
        n = self.nkv(wv)
        return n if n < 16 else 0

    @property
    def xcd_rows(self):
        return self.h // 8 if (self.xcd and self.h % 8 == 0) else 0

    @property
    def scale(self):
        """the fp32 value the kernel computes"""
        return float(np.float32(1.0) / np.sqrt(np.float32(C // self.heads)))


def block_row(case, b, exchanged=False):
    """the row block b of the grid works on (rowattn.hip: the XCD placement); exchanged: img and yl swapped (a wrong kernel)"""
    xr = case.xcd_rows
    if not xr:
        return b
    x, k = b & 7, b >> 3
    yl, img = (k % case.nimg, k // case.nimg) if exchanged else (k // case.nimg, k % case.nimg)
    return img * case.h + x * xr + yl


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    for i, w in enumerate(WIDTHS):
        for heads in (1, 2):
            for cross in (True, False):
                j = len(out)
                regime = "full" if (i + heads + cross) % 2 == 0 else "route"
                nimg = (2, 4, 6)[j % 3] if cross else (1, 3, 2, 4)[(j // 2) % 4]
                h = 1 + (j // 3) % 3
                ln_out = (j // 2 + i) % 2 == 0
                xs = X_STRIDES[(j + i) % 3]
                os_ = OUT_STRIDES[(j // 2 + j // 5) % 2]
                out.append(Case(w, heads, cross, nimg, h, regime, ln_out, xs, os_, LN_STRIDE, 1, regime == "full" and w >= 33 and i % 3 == 0))
    # the probe regimes: the attention stage, the FFN stage and the pass-through (ln_out alone) at one-wave, chunk-boundary and widest rows
    j = 0
    for regime, widths in (("attn", (33, 161, 320)), ("ffn", (8, 160, 225)), ("pass", (31, 257)), ("tail", (33, 161, 288))):
        for w in widths:
            for heads in (1, 2):
                cross = j % 2 == 0
                out.append(Case(w, heads, cross, (2, 4)[j % 2] if cross else (1, 3)[(j // 2) % 2], 1 + j % 3, regime, regime == "pass" or j % 2 == 1,
                                X_STRIDES[j % 3], OUT_STRIDES[(j // 2) % 2], LN_STRIDE, 1, False))
                j += 1
    # the XCD placement: h a multiple of 8, the hint on and off, in the route regime (a permuted row is plainly another row)
    for j, (h, nimg) in enumerate((h, nimg) for h in (8, 16) for nimg in (2, 4, 6)):
        heads = 1 + j % 2                                                            # h = 16 (the map permutes): two heads, one, two
        for xcd in (1, 0):
            out.append(Case(40 if heads == 1 else 33, heads, j % 3 != 1, nimg, h, "route", j % 2 == 1, X_STRIDES[j % 3], OUT_STRIDES[j % 2], LN_STRIDE, xcd, False))
    return tuple(out)


def existing_case(nimg, h, w, heads, cross, ln_out):
    """a shape of tests/test_hip_rowattn.py in the full regime"""
    return Case(w, heads, cross, nimg, h, "full", ln_out, 128, 128, 128, 1, False)


# ---- plain operands ------------------------------------------------------------------------------------------------------------------------
Ops = collections.namedtuple("Ops", "W b wsum gout bout")      # W: six (128, 128) fp16; b: six (128,) fp32; wsum: four (q, k, v, ffn.0); ln_out affine
NAMES = ("q", "k", "v", "proj", "ffn0", "ffn2")


def fold(w, b, gamma=None, beta=None):
    """One linear layer behind a pre-LayerNorm with affine (gamma, beta) -> (fp16 weight, fp32 bias or None) of the same layer behind the
    LayerNorm WITHOUT affine: W (n gamma + beta) + b = (W gamma) n + (W beta + b).  No affine: the layer as it is (the engine's case)."""
    w = w.float()
    if gamma is not None:
        b = (b.float() if b is not None else 0.0) + w @ beta.float()
        w = w * gamma.float()[None, :]
    return w.to(torch.float16).contiguous(), (b.float().contiguous() if b is not None else None)


def make_ops(layers, pre_attn=None, pre_ffn=None, ln_affine=None):
    """layers: six (weight, bias or None) in NAMES order, fp32; pre_attn / pre_ffn: (gamma, beta) of the two pre-LayerNorms or None."""
    W, b = [], []
    for name, (w, bb) in zip(NAMES, layers):
        aff = pre_attn if name in ("q", "k", "v") else pre_ffn if name == "ffn0" else None
        wf, bf = fold(w, bb, *(aff or (None, None)))
        W.append(wf)
        b.append(bf)
    wsum = tuple(W[i].float().sum(1).contiguous() for i in (0, 1, 2, 4))
    g, bo = ln_affine if ln_affine is not None else (None, None)
    return Ops(tuple(W), tuple(b), wsum, g, bo)


def packed(ops, device="cpu"):
    """what the entry takes: (768, 128) fp16 in the row_attn packing, (12, 128) fp32"""
    wts = pack.rowattn_pack(torch.cat(ops.W, 0))
    vec = pack.rowattn_vectors(ops.wsum, ops.b, (ops.gout, ops.bout) if ops.gout is not None else None)
    return wts.to(device).contiguous(), vec.to(device).contiguous()


@functools.lru_cache(maxsize=None)
def operands(regime, heads):
    g = torch.Generator().manual_seed(1300 + 17 * heads + (regime == "route") + 2 * (regime in PROBES))   # (tail: 2)
    rn = lambda *s: torch.randn(*s, generator=g)                                    # noqa: E731
    gout, bout = 1.0 + 0.2 * rn(C), 0.2 * rn(C)
    if regime == "full":
        raw = [rn(C, C) / math.sqrt(C) for _ in range(6)]
        bias = [None, None, 0.3 * rn(C), 0.3 * rn(C), 0.3 * rn(C), 0.3 * rn(C)]
        pre_attn = (1.0 + 0.2 * rn(C), 0.2 * rn(C))
        pre_ffn = (1.0 + 0.2 * rn(C), 0.2 * rn(C))
        return make_ops(list(zip(raw, bias)), pre_attn, pre_ffn, (gout, bout))
    if regime in ("attn", "ffn", "pass"):                                            # the full regime's layers with a stage made transparent
        raw = [rn(C, C) / math.sqrt(C) for _ in range(6)]
        bias = [None, None, 0.3 * rn(C), 0.3 * rn(C), 0.3 * rn(C), 0.3 * rn(C)]
        pre_attn = (1.0 + 0.2 * rn(C), 0.2 * rn(C))
        pre_ffn = (1.0 + 0.2 * rn(C), 0.2 * rn(C))
        if regime == "attn":
            raw[3], bias[3] = torch.eye(C), None                                     # proj: the exact identity
        else:
            raw[3], bias[3] = torch.zeros(C, C), None                                # ffn, pass: z' = x exactly
        if regime != "ffn":
            raw[5], bias[5] = torch.zeros(C, C), None                                # attn, pass: the FFN adds an exact zero
        return make_ops(list(zip(raw, bias)), pre_attn, pre_ffn, (gout, bout))
    d, a = C // heads, ROUTE_A[heads]
    wq, wk = torch.zeros(C, C), torch.zeros(C, C)
    for hd in range(heads):
        for e in range(d // 2):
            wq[hd * d + e, hd * d + e] = a                                          # q dims [0, d / 2) of a head: its query code
            wk[hd * d + e, hd * d + d // 2 + e] = a                                 # k dims [0, d / 2): its key code
    eye = torch.eye(C)
    layers = [(wq, 0.3 * rn(C)), (wk, 0.3 * rn(C)), (eye, 0.3 * rn(C)), (eye, None), (rn(C, C) / math.sqrt(C), 0.3 * rn(C)), (torch.zeros(C, C), None)]
    if regime == "tail":
        sixteenths = lambda lo, hi: torch.randint(lo, hi + 1, (C,), generator=g).float() / 16                   # noqa: E731
        layers[2] = (torch.zeros(C, C), sixteenths(-8, 8))                           # v = c for every key
        layers[3] = (2.0 * eye[(torch.arange(C) + TAIL_SHIFT) % C], sixteenths(1, 16) * (1 - 2 * torch.randint(0, 2, (C,), generator=g).float()))
        layers[5] = (rn(C, C) / math.sqrt(C), 0.3 * rn(C))
    return make_ops(layers, None, None, (gout, bout))


def ops_of(case):
    return operands(case.regime, case.heads)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
Inputs = collections.namedtuple("Inputs", "buf x base pi")      # buf (n + 2, xs) fp16; x its (rows, w, 128) view; base: x's offset in buf; pi: route map


def src_image(case, img, variant=None):
    if not case.cross:
        return img
    if variant == "cross_roll_one":
        return (img + 1) % case.nimg
    if variant == "both_left":
        return img % (case.nimg // 2)
    return (img + case.nimg // 2) % case.nimg


def src_rows(case, variant=None):
    return torch.tensor([src_image(case, r // case.h, variant) * case.h + r % case.h for r in range(case.rows)])


def rm2_codes(m, n, g):
    """n distinct codewords of the second-order Reed-Muller code RM(2, m) as +-1 rows of length 2^m.  Its minimum distance is 2^(m - 2): two
    different codewords agree in at most three quarters of their positions, so their dot product is at most 2^m / 2 against 2^m of a
    codeword with itself"""
    pts = torch.arange(2 ** m)
    v = [(pts >> i) & 1 for i in range(m)]
    basis = torch.stack([torch.ones_like(pts)] + v + [v[i] * v[j] for i in range(m) for j in range(i + 1, m)])
    k = basis.shape[0]
    msgs = torch.randperm(2 ** k, generator=g)[:n]
    bits = (msgs[:, None] >> torch.arange(k)[None, :]) & 1
    return (1 - 2 * ((bits @ basis) % 2)).float()


def route_targets(case):
    w = case.w
    ks = [0, w - 1]
    for t in range(case.ntile):
        ks += [32 * t, min(32 * t + 31, w - 1)]
    ks += [159, 160]
    return [k for i, k in enumerate(ks) if 0 <= k < w and k not in ks[:i]]


def route_map(case, g):
    """pi[row, head, i]: the key query i of the row is aimed at"""
    w, last0 = case.w, 32 * (case.ntile - 1)
    last = sorted({last0, w - 1, (last0 + w - 1) // 2})
    tg = route_targets(case)
    pi = torch.empty(case.rows, case.heads, w, dtype=torch.long)
    for r in range(case.rows):
        for hd in range(case.heads):
            p = torch.randperm(w, generator=g)
            for i in range(0, w, 4):
                p[i] = last[(i // 4 + hd + r) % len(last)]
            for i in range(1, w, 4):
                p[i] = tg[(i // 4 + 3 * hd + r) % len(tg)]
            pi[r, hd] = p
    return pi


def _ln32(t):
    t = t.float()
    m = t.mean(-1, keepdim=True)
    return (t - m) * torch.rsqrt(t.var(-1, unbiased=False, keepdim=True) + EPS)


def _fill(case):
    nimg, h, w, heads = case.nimg, case.h, case.w, case.heads
    g = torch.Generator().manual_seed(((w * 7 + heads) * 11 + nimg) * 13 + h * 3 + case.cross + 100 * (case.regime == "route") + 200 * (case.regime == "tail"))
    rn = lambda *s: torch.randn(*s, generator=g)                                    # noqa: E731
    rows = case.rows
    src = src_rows(case)
    if case.regime in ROUTED:
        d = C // heads
        n = d // 4                                                                   # code length: 32 (one head) or 16 (two)
        pi = route_map(case, g)
        kc = torch.stack([torch.stack([rm2_codes(n.bit_length() - 1, w, g) for _ in range(heads)], 1) for _ in range(rows)])   # (rows, w, heads, n)
        x = torch.empty(rows, w, heads, d)
        x[..., 2 * n:3 * n], x[..., 3 * n:] = kc, -kc
        for r in range(rows):
            for hd in range(heads):
                qc = kc[int(src[r]), pi[r, hd], hd]
                x[r, :, hd, :n], x[r, :, hd, n:2 * n] = qc, -qc
        amp = torch.tensor(ROUTE_AMPS)[(torch.arange(w)[None, :] + torch.arange(rows)[:, None]) % 3]
        return (x.reshape(rows, w, C) * amp[..., None]).to(torch.float16), pi
    if case.regime == "pass":
        return (64.0 + 0.0625 * torch.randint(0, 7, (rows, w, C), generator=g)).to(torch.float16), None
    base = rn(nimg, h, w, C)
    if nimg > 1:                                                                     # correlated left / right rows, as tests/test_hip_rowattn.py has them
        base[nimg // 2:] = 0.7 * base[: nimg - nimg // 2].roll(3, 2) + 0.3 * base[nimg // 2:]
    base = base.reshape(rows, w, C)
    t = torch.arange(w)[None, :]
    line = (torch.arange(rows) % h)[:, None]
    off = torch.tensor(OFFS)[(t + 2 * line) % 3][..., None]
    sc = torch.tensor(SCALES)[(t + line) % 2][..., None]
    x16 = (off + sc * base).to(torch.float16)
    # every tenth query aimed at key w - 1 of its source row
    ops = ops_of(case)
    wq, wk, bk = ops.W[0].float(), ops.W[1].float(), ops.b[1]
    kl = _ln32(x16[src, w - 1]) @ wk.T + bk                                         # (rows, C): key w - 1 of each row's source
    grad = kl @ wq                                                                   # d logit / d LN(x)
    ghat = (grad - grad.mean(-1, keepdim=True)) / grad.std(-1, unbiased=False, keepdim=True)
    qi = torch.arange(3, w - 1, 10)
    if qi.numel():
        aimed = 0.6 * base[:, qi] + 0.8 * ghat[:, None, :]
        x16[:, qi] = (off[:, qi] + sc[:, qi] * aimed).to(torch.float16)
    x16[0, w // 2] = 1.5
    if case.hot:
        x16[rows - 1, 1] = HOT
    return x16, None


@functools.lru_cache(maxsize=4)
def inputs(case, device="cpu"):
    """built once and shared; nothing may write into them"""
    x16, pi = _fill(case)
    n = case.rows * case.w
    pad = (case.xs - C) // 8 * 4
    buf = torch.full((n + 2, case.xs), GUARD_X, dtype=torch.float16)
    buf[1:-1, pad:pad + C] = x16.reshape(n, C)
    buf = buf.to(device)
    x = buf[1:-1, pad:pad + C].view(case.rows, case.w, C) if case.xs == C else buf[1:-1].view(case.rows, case.w, case.xs)[..., pad:pad + C]
    return Inputs(buf, x, case.xs + pad, pi)


def gather_rows(case, inp, rows, pitch=None):
    """(len(rows), w, 128) float64 read from the buffer as the kernel addresses it: base + row * pitch + token * x_stride + channel"""
    dev = inp.buf.device
    pitch = case.w * case.xs if pitch is None else pitch
    idx = (inp.base + rows.to(dev)[:, None, None] * pitch + torch.arange(case.w, device=dev)[None, :, None] * case.xs
           + torch.arange(C, device=dev)[None, None, :])
    return inp.buf.flatten()[idx].double()


# ---- float64 reference ---------------------------------------------------------------------------------------------------------------------
def _ln64(t, eps):
    m = t.mean(-1, keepdim=True)
    return (t - m) / torch.sqrt(t.var(-1, unbiased=False, keepdim=True) + eps)


def _gelu64(t):
    return 0.5 * t * (1.0 + torch.erf(t * (0.5 ** 0.5)))


def _lin64(t, ops, i):
    y = t @ ops.W[i].to(t.device).double().T
    return y + ops.b[i].to(t.device).double() if ops.b[i] is not None else y


def _heads(t, heads):
    return t.reshape(t.shape[0], t.shape[1], heads, -1).transpose(1, 2)


def logits64(case, device="cpu"):
    """(rows, heads, w, w) float64 logits in the log2 domain (score * scale * log2 e)"""
    inp, ops = inputs(case, device), ops_of(case)
    z = gather_rows(case, inp, torch.arange(case.rows))
    s = z[src_rows(case).to(z.device)]
    q, k = _lin64(_ln64(z, EPS), ops, 0), _lin64(_ln64(s, EPS), ops, 1)
    return _heads(q, case.heads) @ _heads(k, case.heads).transpose(-1, -2) * (case.scale * LOG2E)


Ref = collections.namedtuple("Ref", "out ln pre qkv_max z1")    # pre: the FFN pre-activation; qkv_max: the largest |q|, |k| or |v|; z1: z'


@functools.lru_cache(maxsize=4)
def reference(case, device="cpu"):
    inp, ops = inputs(case, device), ops_of(case)
    z = gather_rows(case, inp, torch.arange(case.rows))
    s = z[src_rows(case).to(z.device)]
    q, k, v = _lin64(_ln64(z, EPS), ops, 0), _lin64(_ln64(s, EPS), ops, 1), _lin64(_ln64(s, EPS), ops, 2)
    a = torch.softmax(_heads(q, case.heads) @ _heads(k, case.heads).transpose(-1, -2) * case.scale, -1)
    o = (a @ _heads(v, case.heads)).transpose(1, 2).reshape(z.shape)
    z1 = z + _lin64(o, ops, 3)
    pre = _lin64(_ln64(z1, EPS), ops, 4)
    out = z1 + _lin64(_gelu64(pre), ops, 5)
    ln = None
    if case.ln_out:
        ln = _ln64(out, LN_OUT_EPS) * ops.gout.to(z.device).double() + ops.bout.to(z.device).double()
    return Ref(out, ln, pre, max(float(t.abs().max()) for t in (q, k, v)), z1)


# ---- emulation of the kernel's arithmetic, and wrong variants of it ----------------------------------------------------------------------
VARIANTS = ("ragged_last_from_neighbour", "padding_unmasked", "mask_off_by_one", "no_rescale_at_chunk", "no_rescale_in_tile", "head1_sum_of_head0",
            "scale_c", "cross_roll_one", "both_left", "xcd_exchanged", "vstat_wrong_token", "variance_unclamped", "q_bias_dropped",
            "proj_bias_dropped", "residual_from_o", "residual2_from_x", "ln_out_onepass_unrounded", "cols_unrelabelled", "pitch_w128")


def applies(variant, case):
    """does the case have the feature the variant breaks?"""
    ragged = case.w % 32 != 0
    full = case.regime == "full"
    return {
        "ragged_last_from_neighbour": ragged, "padding_unmasked": ragged, "mask_off_by_one": ragged,
        "no_rescale_at_chunk": case.nchunk > 1, "no_rescale_in_tile": case.ntile > 1,
        "head1_sum_of_head0": case.heads == 2, "scale_c": case.heads == 2,
        "cross_roll_one": case.cross, "both_left": case.cross, "xcd_exchanged": case.xcd_rows > 0,
        "vstat_wrong_token": True, "variance_unclamped": bool(case.hot), "q_bias_dropped": True, "proj_bias_dropped": full or case.regime == "tail",
        "residual_from_o": True, "residual2_from_x": full or case.regime == "tail", "ln_out_onepass_unrounded": bool(case.ln_out),
        "cols_unrelabelled": True, "pitch_w128": case.xs != C,
    }[variant]


def exempt(variant, case):
    """a case the variant's feature applies to but the variant cannot change: the rule, or None.  (A wrong K bias is no variant at all: it
    shifts every logit of a query by the same q . bk, which the softmax cancels in exact arithmetic.)"""
    if variant == "cross_roll_one" and case.nimg == 2:
        return "two images: (n + 1) % nimg is (n + nimg / 2) % nimg"
    if variant == "q_bias_dropped" and case.regime in ROUTED:
        return "route tokens: the magnet's lead of more than 40 does not depend on the q bias; the probabilities stay 0 and 1"
    if variant == "ln_out_onepass_unrounded" and case.regime != "pass":
        return "rows of |mean| / std below 10: the one-pass variance in fp32 is as good as the two-pass one, and half an ulp of the sum is inside the bound"
    return None


def ulp16(v):
    """the spacing of fp16 at magnitude |v| (float64 tensor)"""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -14))) - 10)


class Rounder:
    """float64 -> the fp16 value the kernel stores (through fp32, as from_f32 rounds), optionally moved to a neighbour"""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed) if seed is not None else None

    def __call__(self, t, exact=False):
        r = t.float().to(torch.float16).double()
        if self.g is None or exact:
            return r
        u = torch.rand(r.shape, generator=self.g).to(r.device)
        d = (u >= 0.875).double() - (u < 0.125).double()
        d = torch.where((r == 0) | ~torch.isfinite(r), torch.zeros_like(d), d)
        return (r + d * ulp16(r)).float().to(torch.float16).double()


_f32 = lambda t: t.float().double()                                                 # noqa: E731
_HALF_ORDER = torch.tensor([[16 * s + 8 * u + 4 * hi + e for s in range(8) for u in range(2) for e in range(4)] for hi in range(2)])


def ln_stats(x, eps, clamp=True, order=None):
    """mean and rstd of the last axis as ra_ln_stats takes them: each half-wave runs over its 64 channels in fragment order, two at a time
    (v_dot2: the two products and the running sum rounded once to fp32), the halves are added, the variance is fma(-mean, mean, q / C),
    clamped at 0.  x: float64 holding fp16 (or fp32) values.  order: (2, C / 2) channel indices, the order in which each half-wave of another
    kernel takes a row of another width (tests/k9_cases.py); the width is that of x, and 1 / C is the fp32 constant the kernels multiply by."""
    o = (_HALF_ORDER if order is None else order).to(x.device)
    width = x.shape[-1]
    assert o.numel() == width, (tuple(o.shape), width)
    inv = float(np.float32(1.0) / np.float32(width))
    xs = x[..., o]                                                                   # (..., 2, C / 2)
    s = torch.zeros(xs.shape[:-1], dtype=torch.float64, device=x.device)
    q = torch.zeros_like(s)
    for p in range(o.shape[1] // 2):
        a, b = xs[..., 2 * p], xs[..., 2 * p + 1]
        s = _f32(s + (a + b))
        q = _f32(q + (a * a + b * b))
    s, q = _f32(s.sum(-1)), _f32(q.sum(-1))
    mean = _f32(s * inv)
    var = _f32(_f32(q * inv) - mean * mean)
    if clamp:
        var = var.clamp(min=0.0)
    rstd = _f32(1.0 / torch.sqrt(_f32(var + float(np.float32(eps)))))
    return mean[..., None], rstd[..., None]


def emulate(case, variant=None, flips=None, device="cpu"):
    """-> (out, ln or None): (rows, w, 128) float64 tensors holding fp16 values; NaN where a wrong variant never writes"""
    inp, ops = inputs(case, device), ops_of(case)
    rd = Rounder(flips)
    w, heads, rows = case.w, case.heads, case.rows
    d = C // heads
    dev = inp.buf.device
    pitch = w * C if variant == "pitch_w128" else None
    z = gather_rows(case, inp, torch.arange(rows), pitch)
    s = gather_rows(case, inp, src_rows(case, variant), pitch)
    W = [t.to(dev).double() for t in ops.W]
    if variant == "cols_unrelabelled":                                               # the kernel's k-slot order meets plain columns
        W = [pack.rowattn_cols(t) for t in W]
    b = [(t.to(dev).double() if t is not None else torch.zeros(C, dtype=torch.float64, device=dev)) for t in ops.b]
    if variant == "q_bias_dropped":
        b[0] = torch.zeros_like(b[0])
    if variant == "proj_bias_dropped":
        b[3] = torch.zeros_like(b[3])
    wsum = [t.to(dev).double() for t in ops.wsum]
    clamp = variant != "variance_unclamped"

    def folded(t, i, wi, stats):
        mean, rstd = stats
        return rstd * (t @ W[i].T - mean * wsum[wi]) + b[i]

    zst = ln_stats(z, EPS, clamp)
    sst = ln_stats(s, EPS, clamp)
    q = rd(folded(z, 0, 0, zst))
    k = rd(folded(s, 1, 1, sst))
    vst = sst
    if variant == "vstat_wrong_token":                                               # stat[(r & 3) + 4 hi]: the token's index modulo 8 inside its tile
        tok = torch.arange(w, device=dev)
        wrong = (tok // 32 * 32 + tok % 8).clamp(max=w - 1)
        vst = (sst[0][:, wrong], sst[1][:, wrong])
    v = rd(folded(s, 2, 2, vst))
    # ---- online softmax over 32-key tiles; the padding lanes of the last tile hold copies of token w - 1
    nk = 32 * case.ntile
    kidx = torch.arange(nk, device=dev).clamp(max=w - 1)
    kp, vp = k[:, kidx], v[:, kidx]
    limit = nk if variant == "padding_unmasked" else w - 1 if variant == "mask_off_by_one" else w
    scale = case.scale
    if variant == "scale_c":
        scale = float(np.float32(1.0) / np.sqrt(np.float32(C)))
    scale2 = float(np.float32(scale) * np.float32(LOG2E))
    o = torch.empty_like(z)
    l_head = []
    for hd in range(heads):
        sl = slice(hd * d, (hd + 1) * d)
        m = torch.full((rows, w), -float("inf"), dtype=torch.float64, device=dev)
        l = torch.zeros_like(m)
        acc = torch.zeros(rows, w, d, dtype=torch.float64, device=dev)
        for t in range(case.ntile):
            sc = q[..., sl] @ kp[:, 32 * t:32 * t + 32, sl].transpose(-1, -2)
            if 32 * t + 32 > w:                                                      # the kernel masks only a tile that is not full
                dead = torch.arange(32 * t, 32 * t + 32, device=dev) >= limit
                sc = torch.where(dead[None, None, :], torch.full_like(sc, -float("inf")), sc)
            m_new = torch.maximum(m, sc.max(-1).values * scale2)
            alpha = torch.exp2(m - m_new)
            p = torch.exp2(sc * scale2 - m_new[..., None])
            l = l * alpha + p.sum(-1)
            keep = (variant == "no_rescale_at_chunk" and t > 0 and t % 5 == 0) or (variant == "no_rescale_in_tile" and t % 5 != 0)
            if not keep:
                acc = acc * alpha[..., None]
            acc = acc + rd(p) @ vp[:, 32 * t:32 * t + 32, sl]
            m = m_new
        l_head.append(l)
        ln = l_head[0] if variant == "head1_sum_of_head0" else l
        o[..., sl] = acc / ln[..., None]
    o = rd(o)
    pr = rd(o @ W[3].T + b[3])
    z1 = rd(pr + (o if variant == "residual_from_o" else z), exact=True)
    hid = rd(_gelu64(folded(z1, 4, 3, ln_stats(z1, EPS, clamp))))
    f = rd(hid @ W[5].T + b[5])
    total = f + (z if variant == "residual2_from_x" else z1)
    out = rd(total, exact=True)
    if variant == "ragged_last_from_neighbour":
        out[:, w - 1] = out[:, w - 2]
    ln = None
    if case.ln_out:
        g, bo = ops.gout.to(dev).double(), ops.bout.to(dev).double()
        if variant == "ln_out_onepass_unrounded":
            mean, rstd = ln_stats(_f32(total), LN_OUT_EPS)
            ln = rd((_f32(total) - mean) * rstd * g + bo)
        else:
            mu = out.mean(-1, keepdim=True)
            rs = 1.0 / torch.sqrt(((out - mu) ** 2).mean(-1, keepdim=True) + LN_OUT_EPS)
            ln = rd((out - mu) * rs * g + bo)
    if variant == "xcd_exchanged":                                                   # the rows the wrong map visits are computed; the others never written
        seen = torch.zeros(rows, dtype=torch.bool)
        for blk in range(rows):
            r = block_row(case, blk, exchanged=True)
            if r < rows:
                seen[r] = True
        out[~seen] = float("nan")
        if ln is not None:
            ln[~seen] = float("nan")
    return out, ln


# ---- bounds and the comparator -------------------------------------------------------------------------------------------------------------
def token_bound(ref, members):
    """ulp16(max(1, |R|)) + 2 D_t, D_t = the largest |E_s - R| over the channels of token t and the members"""
    D = torch.stack([(m - ref).abs().amax(-1) for m in members]).amax(0)
    return ulp16(ref.abs().clamp(min=1.0)) + 2.0 * D[..., None]


U24 = 2.0 ** -24
half16 = lambda value, err: 0.5 * ulp16(value.abs() + err)                          # noqa: E731  (half an ulp at the largest magnitude being rounded)


def ln_fold_bound(x, wabs_x, acc, ws, eps=EPS):
    """Elementwise bound of the error of y = rstd (acc - mean ws) + b as the kernel forms it in fp32, BEFORE y is rounded to fp16, against the
    same expression in exact arithmetic.  x (.., C) the token (float64, fp16 values); acc = W . x (.., Cout); wabs_x = |W| . |x|; ws = rowsum(W).
    u = 2^-24, m and v the exact mean and variance of the token, M2 = m^2 + v = mean(x^2).
      sums      each half-wave adds 64 values in a chain and the halves are added: |fl(s) - s| <= (C / 2 + 1) u sum|x|, the same for q = sum x^2:
                  dm = (C / 2 + 1) u mean|x|,   |d(q / C)| <= (C / 2 + 1) u M2
      variance  fl(q / C - mean^2) by one fma: |dvar| <= (C / 2 + 1) u M2 + 2 |m| dm + u M2 <= (1.5 C + 4) u M2, since |m| mean|x| <= M2.
                This is the one-pass form's weakness: relative to v it is (1.5 C + 4) u (m^2 + v) / v, i.e. amplified by 1 + (m / std)^2.
      rstd      (var + eps)^-1/2 with the add rounded (u) and v_rsq_f32 within one ulp (2 u): with r = dvar / (v + eps) < 1
                  rho = (1 - r)^-1/2 - 1 + 3 u        (about r / 2).  A constant token has v = 0 and rstd = eps^-1/2 exactly only if its sums are
                exact (1.5 is; HOT is not: there dvar reaches eps and this bound is void -- the full regime judges such tokens, not this one).
      product   acc is an fp32 chain of C products in any order, (C + 2) u |W| |x|; mean ws, the subtraction, the two fmas: 3 u (|acc| + |m ws|)
      together  |dy| <= rstd [ rho |acc - m ws| + (C + 2) u |W||x| + dm |ws| + 3 u (|acc| + |m ws|) ] (1 + rho) + u |y|
    A perturbation e of the accumulator is amplified by rstd: that is the factor in front.  C is the width of x."""
    C = x.shape[-1]
    m = x.mean(-1, keepdim=True)
    v = x.var(-1, unbiased=False, keepdim=True)
    M2 = m * m + v
    dm = (C / 2 + 1) * U24 * x.abs().mean(-1, keepdim=True)
    r = ((1.5 * C + 4) * U24 * M2 / (v + eps)).clamp(max=0.75)
    rho = (1 - r) ** -0.5 - 1 + 3 * U24
    rstd = (v + eps) ** -0.5
    core = acc - m * ws
    e = rstd * (rho * core.abs() + (C + 2) * U24 * wabs_x + dm * ws.abs() + 3 * U24 * (acc.abs() + (m * ws).abs())) * (1 + rho)
    return e + U24 * (rstd * core).abs()


def ln_out_bound(out, E, g, b, eps=LN_OUT_EPS, half=None):
    """Bound of ln_out (the LayerNorm of the STORED rows, two passes in fp32) against LayerNorm(out) g + b of the reference's rows, when the
    stored rows are within E of out.  n = (o - mu) / sigma: a perturbation d of the row moves n_c by (d_c - mean d) / sigma - n_c dsigma / sigma
    with |dsigma| <= rms(d), so |dn_c| <= (E_c + mean E + |n_c| rms E) / sigma, to first order (second order: the factor 1.02, E << sigma);
    the kernel's own arithmetic is two fp32 chains of C terms and five operations per element, (C + 8) u (|n_c| + 1); the affine and one
    rounding to fp16 follow (half: half an ulp of another I/O dtype, tests/k9_cases.py).  C is the width of out."""
    C = out.shape[-1]
    half = half16 if half is None else half
    mu = out.mean(-1, keepdim=True)
    sig = torch.sqrt(out.var(-1, unbiased=False, keepdim=True) + eps)
    n = (out - mu) / sig
    dn = 1.02 * (E + E.mean(-1, keepdim=True) + n.abs() * torch.sqrt((E * E).mean(-1, keepdim=True))) / sig + (C + 8) * U24 * (n.abs() + 1)
    e = g.abs() * dn + 2 * U24 * (n * g + b).abs()
    return e + half(n * g + b, e)


def route_bound(case, device="cpu"):
    """The route regime's elementwise bound, from the arithmetic alone.  The magnet's logit leads by more than 40 in the log2 domain, so its
    probability is 1, every other one is below 2^-40 and rounds to 0 in fp16 (the smallest fp16 subnormal is 2^-24); what an earlier tile put
    into the accumulator before the magnet arrived is rescaled by alpha <= 2^-40 (at most w keys of weight <= 1: w 2^-40 max|v|); the row sum
    is 1 + w 2^-40.  So o is the kernel's own fp16 v of the magnet key, proj (the exact identity) returns it, and
      out = fp16(v + x),   v = fp16(rstd (s_c - mean) + bv_c):   ln_fold_bound with W = I, half an ulp of v, the leak, half an ulp of the sum."""
    inp, ops = inputs(case, device), ops_of(case)
    z = gather_rows(case, inp, torch.arange(case.rows))
    s = z[src_rows(case).to(z.device)]
    ws = ops.wsum[2].to(z.device).double()
    vex = _lin64(_ln64(s, EPS), ops, 2)
    ev = ln_fold_bound(s, s.abs(), s, ws)
    ev = ev + half16(vex, ev)                                                        # per key
    ev = ev + case.w * 2.0 ** -40 * vex.abs().amax(1, keepdim=True)
    d = C // case.heads
    pi = inp.pi.to(z.device)
    E = torch.empty_like(z)
    for hd in range(case.heads):
        sl = slice(hd * d, (hd + 1) * d)
        E[..., sl] = torch.gather(ev[..., sl], 1, pi[:, hd, :, None].expand(-1, -1, d))
    ref = reference(case, device)
    return E + half16(ref.out, E)


def _fold_layer(t, ops, i, wi):
    """-> (the exact output of LN-folded layer i on tokens t, the bound of the kernel's fp16 value of it)"""
    dev = t.device
    w = ops.W[i].to(dev).double()
    e = ln_fold_bound(t, t.abs() @ w.abs().T, t @ w.T, ops.wsum[wi].to(dev).double())
    y = _lin64(_ln64(t, EPS), ops, i)
    return y, e + half16(y, e)


def attn_probe_bound(case, device="cpu"):
    """The attention probe's elementwise bound.  proj is the exact identity and the FFN adds an exact zero: out = fp16(o + x).
    q, k, v: ln_fold_bound (the K5-style (C + 2) u |W||x| inside it) and half an ulp each: eq, ek, ev.  The logits move by at most
    dt_ik = scale (eq_i . |k_k| + |q_i| . ek_k + eq_i . ek_k), which multiplies p_k by at most e^dt: K4's relative error e_k of the kernel's
    p_k (k4_cases.weights64: fp32 score accumulation, the fma, v_exp_f32) becomes (1 + e_k) e^dt - 1, and K4's bound (k4_cases.bound_terms: P
    rounded to fp16, fp32 accumulation of N and L in any order, the rescales, the output's rounding) holds with it.  The values' own error
    adds sum_k a_k (1 + e_k) ev_k / (1 - dL).  Half an ulp of the residual sum."""
    import k4_cases as K4
    inp, ops = inputs(case, device), ops_of(case)
    z = gather_rows(case, inp, torch.arange(case.rows))
    s = z[src_rows(case).to(z.device)]
    hs = lambda t: _heads(t, case.heads)                                             # noqa: E731
    (q, eq), (k, ek), (v, ev) = _fold_layer(z, ops, 0, 0), _fold_layer(s, ops, 1, 1), _fold_layer(s, ops, 2, 2)
    q, eq, k, ek, v, ev = hs(q), hs(eq), hs(k), hs(ek), hs(v), hs(ev)
    a, e = K4.weights64(q, k, case.scale)
    dt = case.scale * (eq @ k.abs().transpose(-1, -2) + q.abs() @ ek.transpose(-1, -2) + eq @ ek.transpose(-1, -2))
    e = (1 + e) * torch.exp(dt) - 1
    ref_o = a @ v
    b = K4.bound_terms(a, e, v, ref_o, case.w, True)
    dL = (a * e).sum(-1, keepdim=True) * (1 + (case.w + K4.TAIL_OPS) * K4.U24) + (case.w + K4.TAIL_OPS) * K4.U24
    b = b + ((a * (1 + e)) @ ev) / (1 - dL)
    E = b.transpose(1, 2).reshape(z.shape)
    return E + half16(reference(case, device).out, E)


def ffn_probe_bound(case, device="cpu"):
    """The elementwise bound of the FFN stage on a z' that the kernel holds EXACTLY as the reference has it: out = fp16(z' + f), two layers deep:
      pre   ln_fold_bound of ffn.0 on z'                                           hid   GELU: Lipschitz 1.13, k5_cases.GELU_ABS, one fp16 ulp for the
      f     |W2| e_hid + (C + 2) u (|W2| |hid| + |b2|), half an ulp                      fast form (tests/test_gelu16_cpu.py), half an ulp of the store
      out   half an ulp of the sum
    ffn   proj and its bias are zero: z' = x.
    tail  the route regime's q and k make every probability 0 or 1 (the leak is below w 2^-40, see route_bound); the V layer is zero with a
          bias c of sixteenths, |c| <= 1/2, so v = c for every key and o = fp16(c (1 + 2^-30)) = c whichever key was taken; proj is twice a
          rotation of the channels plus a bias of non-zero sixteenths, |b| <= 1: one exact product per output, pr = 2 c' + b a multiple of
          1/16 within +-2; x is +-1/2, +-1 or +-2: z' = x + pr is a multiple of 1/16 within +-4, an fp16 value, no rounding anywhere.
          reference().z1 is that value (the CPU tests assert it is an fp16 value); a wrong proj, bias or residual moves z' by at least 1/16,
          which the identity path carries to out."""
    import k5_cases as K5
    ops = ops_of(case)
    x = reference(case, device).z1
    w0, w2 = ops.W[4].to(x.device).double(), ops.W[5].to(x.device).double()
    pre = _lin64(_ln64(x, EPS), ops, 4)
    e = ln_fold_bound(x, x.abs() @ w0.abs().T, x @ w0.T, ops.wsum[3].to(x.device).double())
    g = _gelu64(pre)
    e = K5.LIPSCHITZ[K5.ACT_GELU] * e + K5.GELU_ABS["float16"]
    e = e + ulp16(g.abs() + e)
    e = e + half16(g, e)
    f = _lin64(g, ops, 5)
    ef = e @ w2.abs().T + (C + 2) * U24 * ((g.abs() + e) @ w2.abs().T + ops.b[5].to(x.device).double().abs())
    ef = ef + half16(f, ef)
    return ef + half16(x + f, ef)


EXACT = 2.0 ** -30                                                                   # the bound of an output that must equal the reference


def probe_bound(case, device="cpu"):
    if case.regime == "attn":
        return attn_probe_bound(case, device)
    if case.regime in ("ffn", "tail"):
        return ffn_probe_bound(case, device)
    return torch.full_like(reference(case, device).out, EXACT)                       # pass: out is x, bit for bit


Judge = collections.namedtuple("Judge", "out bound ln ln_bound members")


@functools.lru_cache(maxsize=4)
def judge(case, device="cpu"):
    """full: the reference, the nine emulations (round to nearest and eight flipped) and the per-token bounds built from them;
    route: the reference, the analytic bound and the round-to-nearest emulation"""
    ref = reference(case, device)
    if case.regime != "full":
        ops = ops_of(case)
        bound = route_bound(case, device) if case.regime == "route" else probe_bound(case, device)
        lb = ln_out_bound(ref.out, bound, ops.gout.to(device).double(), ops.bout.to(device).double()) if case.ln_out else None
        return Judge(ref.out, bound, ref.ln, lb, [emulate(case, None, None, device)])
    members = [emulate(case, None, None, device)] + [emulate(case, None, sd, device) for sd in FLIP_SEEDS]
    bound = token_bound(ref.out, [m[0] for m in members])
    lb = token_bound(ref.ln, [m[1] for m in members]) if case.ln_out else None
    return Judge(ref.out, bound, ref.ln, lb, members)


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


def verdict(case, out, ln, device="cpu"):
    """-> [(what, Result)] of a kernel's (or an emulation's) outputs under the case's bounds"""
    j = judge(case, device)
    res = [("out", compare(out, j.out, j.bound))]
    if case.ln_out:
        res.append(("ln", compare(ln, j.ln, j.ln_bound)))
    return res


def line(case, what, res):
    r, tok, ch = res.where
    return (f"{case.id:52s} w {case.w:3d} waves {case.nwv:2d} chunks {case.nchunk} {case.regime:5s} {what:3s} max err {res.err:.3e}  bound {res.bound:.3e}"
            f"  ratio {res.ratio:.3f}  over 1: {res.nbad} of {res.n}  at (image {r // case.h}, line {r % case.h}, token {tok}, channel {ch})"
            f"  {'ok' if res.ratio <= 1 else 'FAIL'}")
