"""Module-level fp16 parity (test infrastructure, imports without a GPU): the comparator ``judge`` and the case inputs shared by
tests/test_module_parity_cpu.py (the comparator's power, on the CPU) and tests/test_hip_fp16_modules.py (every fp16 module form of the
engine against the oracle, teacher-forced at its own boundary).

Per case three outputs of the same module on the same inputs (``x16``: the input rounded to fp16, as the engine's activations are;
``sd16``: every weight of two or more dimensions rounded to fp16, as the engine packs them -- biases and norm affines stay fp32):

* ``y32``  the oracle in fp32,
* ``y16e`` the oracle's emulation of the reference's fp16 autocast deployment (``O.precision("fp16")``),
* ``yh``   the engine method under test.

The yardstick is the emulation's own distance from fp32, computed from the oracle alone.  The engine rounds to fp16 at fewer points than
autocast does (fp32 accumulators, fp32 epilogues, one rounding per launch) and merges some layers in fp32 before rounding them (stacked
Q | K | V, the pre-LayerNorm row sums ``wsum`` of the folded ``W.x - mu.sum(w)``): both keep it closer to fp32 than the emulation, so a
kernel that is subtly wrong shows up as a ratio well above one (measured: see the bounds below).
"""
from __future__ import annotations

import contextlib
from typing import Callable, Dict, Iterator, Mapping, Optional, Tuple

import torch

from oracle import s2m2_oracle as O

# Measured over the 441 GPU cases (profiles/r07/fp16_modules.txt): the largest hip / emulation ratios are median 1.01, p99 1.01, max 1.48
# (L, a 2-D block of the refiner U-Net on seeded inputs): at module level the engine sits at or below the emulation's distance from fp32,
# so the bounds leave a margin of ~1.2x at the quantiles and ~1.35x at the maximum for the worst case, and far more for the rest.
Q_RATIO = 1.25        # median and p99 of |yh - y32| against the same quantiles of |y16e - y32|
MAX_RATIO = 2.0       # max |yh - y32| against max |y16e - y32|
FLOOR = 2.0 ** -16    # added to both bounds, relative to the RMS of y32 (exact outputs: the emulation's quantiles can be 0)
ULPS = 4              # ... and at most ULP_FRAC of the elements further than ULPS fp16 ulps of max(|y32|, 2^-14) from y32
ULP_FRAC = 1e-3       # -- or, where the emulation itself has more such elements, no more than it has.  Autocast rounds every op's output,
#                       and an element whose value comes out of a cancellation keeps the absolute error of the larger terms: measured
#                       fractions of the emulation beyond 4 ulps (S weights, seeded inputs): BasicAttnBlock 9.7 % (~20 rounding points:
#                       q, k, v, probabilities, attention output, proj, residual sum, FFN hidden, GELU, FFN output, sum; twice), ConvBlock
#                       6.6 % (7: the two 3x3 outputs, GELU, the 1x1 outputs, the sum), GlobalAttnBlock with PE 6.6 %.  The HIP numbers
#                       the bound was set against are in profiles/r07/fp16_modules.txt.


def round16(x: torch.Tensor) -> torch.Tensor:
    return x.detach().float().half().float()


def sd16(sd: Mapping[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The state_dict as the engine packs it: weights with >= 2 dims rounded to fp16, biases / norm affines fp32."""
    return {k: (round16(v) if v.dim() >= 2 else v.detach().float().clone()) for k, v in sd.items()}


def oracle_pair(fn: Callable, *args):
    """(fn in fp32, fn in the fp16 autocast emulation) on the same inputs."""
    with torch.no_grad():
        with O.precision("fp32"):
            y32 = fn(*args)
        with O.precision("fp16"):
            y16e = fn(*args)
    return y32, y16e


def nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 3, 1, 2).contiguous()


def fp16_ulp(a: torch.Tensor) -> torch.Tensor:
    """one fp16 ulp at max(|a|, 2^-14) (normal range: 2^(floor(log2 |a|) - 10))"""
    a = a.abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def _kth(e: torch.Tensor, q: float) -> float:
    n = e.numel()
    return float(e.kthvalue(max(1, min(n, int(round(q * n))))).values)


def error_stats(y: torch.Tensor, y32: torch.Tensor, keep: Optional[torch.Tensor] = None) -> Dict[str, float]:
    e = (y.float() - y32.float()).abs().reshape(-1)
    over = e > ULPS * fp16_ulp(y32.float()).reshape(-1)
    if keep is not None:
        e, over = e[keep.reshape(-1)], over[keep.reshape(-1)]
    return dict(median=_kth(e, 0.5), p99=_kth(e, 0.99), max=float(e.max()), ulp_frac=float(over.float().mean()))


class Verdict:
    def __init__(self, ok: bool, msg: str, hip: Dict[str, float], emu: Dict[str, float]):
        self.ok, self.msg, self.hip, self.emu = ok, msg, hip, emu

    def __bool__(self):
        return self.ok

    def ratios(self) -> Dict[str, float]:
        return {k: self.hip[k] / max(self.emu[k], 1e-30) for k in ("median", "p99", "max")}

    def row(self) -> str:
        h, e = self.hip, self.emu
        return ("hip  med %.3g p99 %.3g max %.3g ulp>4 %.2g | emu  med %.3g p99 %.3g max %.3g ulp>4 %.2g"
                % (h["median"], h["p99"], h["max"], h["ulp_frac"], e["median"], e["p99"], e["max"], e["ulp_frac"]))


def _profile(err: torch.Tensor, dim: int, group: int) -> str:
    """max error per group of ``group`` indices along ``dim`` of an (n, h, w, c) error tensor"""
    m = err.amax(dim=tuple(d for d in range(4) if d != dim))
    n = m.numel()
    return " ".join("%d:%.2g" % (i, float(m[i:i + group].max())) for i in range(0, n, group))


def judge(yh: torch.Tensor, y32: torch.Tensor, y16e: torch.Tensor, name: str = "", keep: Optional[torch.Tensor] = None,
          ulp_ratio: float = 1.0) -> Verdict:
    """All three (n, h, w, c).  Passes iff yh is finite; median / p99 of |yh - y32| <= Q_RATIO x those of |y16e - y32| + floor; max <=
    MAX_RATIO x the emulation's max + floor; at most ULP_FRAC of the elements beyond ULPS fp16 ulps of y32.  The message of a failure
    names the (n, h, w, c) of the largest error and the error profile along w (tiles of 32 tokens) and c (groups of 16 channels).
    ``keep`` (optional bool tensor of the same shape, computed from the oracle alone): the statistics of both sides are taken over its
    True elements only (an output with a discontinuity: the elements within the emulation's own reach of the jump are left out);
    every element must still be finite.  ``ulp_ratio``: a module kind's own bound on its fraction beyond ULPS ulps relative to the
    emulation's (default 1.0: no more than the emulation has), for kinds that round at as many points as autocast does -- set where
    the kind is defined, from its measured worst ratio."""
    yh, y32, y16e = yh.detach().float().cpu(), y32.detach().float().cpu(), y16e.detach().float().cpu()
    if yh.shape != y32.shape or y16e.shape != y32.shape:
        raise AssertionError(f"{name}: shapes {tuple(yh.shape)} / {tuple(y32.shape)} / {tuple(y16e.shape)}")
    if keep is not None:
        keep = keep.detach().cpu().bool()
        if keep.shape != y32.shape or not bool(keep.any()):
            raise AssertionError(f"{name}: keep mask {tuple(keep.shape)} for outputs {tuple(y32.shape)}, {int(keep.sum())} kept")
    emu = error_stats(y16e, y32, keep)
    if not bool(torch.isfinite(yh).all()):
        bad = (~torch.isfinite(yh)).nonzero()[0].tolist()
        return Verdict(False, f"{name}: {int((~torch.isfinite(yh)).sum())} non-finite elements, first at (n,h,w,c)={bad}", emu, emu)
    hip = error_stats(yh, y32, keep)
    floor = FLOOR * float((y32 if keep is None else y32[keep]).pow(2).mean().sqrt())
    fails = []
    for k in ("median", "p99"):
        if hip[k] > Q_RATIO * emu[k] + floor:
            fails.append(f"{k} {hip[k]:.3g} > {Q_RATIO} x {emu[k]:.3g} + {floor:.2g}")
    if hip["max"] > MAX_RATIO * emu["max"] + floor:
        fails.append(f"max {hip['max']:.3g} > {MAX_RATIO} x {emu['max']:.3g} + {floor:.2g}")
    if hip["ulp_frac"] > max(ULP_FRAC, ulp_ratio * emu["ulp_frac"]):
        fails.append(f"{hip['ulp_frac']:.5g} of the elements beyond {ULPS} fp16 ulps (emulation: {emu['ulp_frac']:.5g}"
                     + (f", bound {ulp_ratio:.4g} x" if ulp_ratio != 1.0 else "") + ")")
    v = Verdict(not fails, "", hip, emu)
    if fails:
        err = (yh - y32).abs() if keep is None else (yh - y32).abs() * keep
        idx = list(torch.unravel_index(err.argmax(), err.shape))
        at = tuple(int(i) for i in idx)
        v.msg = (f"{name}: " + "; ".join(fails) + f"\n  largest error at (n,h,w,c)={at}: hip {float(yh[at]):.5g} fp32 {float(y32[at]):.5g}"
                 f" emu {float(y16e[at]):.5g}\n  max |err| along w (per 32 tokens): {_profile(err, 2, 32)}"
                 f"\n  max |err| along c (per 16 channels): {_profile(err, 3, 16)}\n  {v.row()}")
    return v


# ---- case inputs ----------------------------------------------------------------------------------------------------------------------
def seeded(shape, seed: int, mean: float = 0.0, std: float = 1.0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return round16(torch.randn(*shape, generator=g) * std + mean)


def offset_tokens(shape, seed: int) -> torch.Tensor:
    """regime (c): a per-token mean far above the spread (6 +- 0.5 per token, std 0.5 within), which stresses the folded pre-LayerNorm
    W.x - mu.sum(w) of the direct K9 / K13 / pre-LN 1x1 forms (cancellation of two large terms)"""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    mu = 6.0 + 0.5 * torch.randn(n, 1, h, w, generator=g)
    return round16(mu + 0.5 * torch.randn(n, c, h, w, generator=g))


def peaked_pair(shape, seed: int, shift: int) -> torch.Tensor:
    """regime (b) input: (2B, C, h, w), the right half = the left half moved ``shift`` tokens along w plus a little noise, so that cross
    attention finds sharp matches ``shift`` tokens away (in the last key chunk for the tokens near the row start)"""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    left = torch.randn(n // 2, c, h, w, generator=g)
    right = torch.roll(left, shift, dims=3) + 0.1 * torch.randn(n // 2, c, h, w, generator=g)
    return round16(torch.cat([left, right], 0))


def peaked_sd(sd: Mapping[str, torch.Tensor], block: str, scale: float = 4.0) -> Dict[str, torch.Tensor]:
    """regime (b) weights: the q weights of every attention of ``block`` scaled (softmax rows close to one-hot)"""
    out = dict(sd)
    for k in sd:
        if k.startswith(block + ".") and k.endswith(".attn.q.weight"):
            out[k] = round16(sd[k] * scale)
    return out


@contextlib.contextmanager
def patched(obj, name: str, value) -> Iterator[None]:
    old = getattr(obj, name)
    setattr(obj, name, value)
    try:
        yield
    finally:
        setattr(obj, name, old)


def capture_boundaries(sd: Mapping[str, torch.Tensor], x: torch.Tensor, ntr: int, refine_iter: int = 0) -> Dict[str, Tuple[torch.Tensor, ...]]:
    """regime (a): the oracle's own fp32 inputs of every module of the trunk (CNN encoder, feature pyramid, transformers) on image
    tensor x (2B, 3, H, W) normalised to [-1, 1] -> {module prefix: its positional tensor arguments}.  refine_iter > 0: the forward goes
    on through DispInit (use_positivity), the refiners, the mask heads and the convex upsampling as O._forward does, and the inputs of
    those modules are recorded under "refine:<kind>" keys (capture_refine)."""
    got: Dict[str, Tuple[torch.Tensor, ...]] = {}

    def rec(fn, nargs):
        def wrapped(sd_, p, *a, **k):
            got.setdefault(p, tuple(t.clone() for t in a[:nargs]))
            return fn(sd_, p, *a, **k)
        return wrapped
    with contextlib.ExitStack() as st, torch.no_grad(), O.precision("fp32"):
        for name, nargs in (("conv_block", 1), ("feature_fusion", 2), ("basic_attn_block", 1), ("global_attn_block", 1), ("unet", 1),
                            ("mrt", 4), ("cnn_encoder", 1), ("_up", 1)):
            st.enter_context(patched(O, name, rec(getattr(O, name), nargs)))
        f4, f2 = O.cnn_encoder(sd, "cnn_backbone", x)
        py = z = O.unet(sd, "feat_pyramid", f4)
        for i in range(ntr):
            z = O.mrt(sd, f"transformer.uformer_list.{i}", *z)
    if refine_iter:                                    # (outside the trunk's patches: the U-Nets of the refiners stay seeded cases)
        B = x.shape[0] // 2
        got.update(capture_refine(sd, x[:B], f2[:B], py[0][:B], z[0].contiguous(), refine_iter))
    return got


def pick(t: torch.Tensor, rows: Optional[int]) -> torch.Tensor:
    """the first ``rows`` rows (full width) of an (n, c, h, w) tensor, or all of it"""
    return t if rows is None or rows >= t.shape[2] else t[:, :, :rows].contiguous()


# ---- the refinement half: GlobalRefiner, ctx / hidden, LocalRefiner iterations, mask heads, convex upsampling ---------------------------
# Each o_* function is the oracle side of one module case (run in fp32 and in the fp16 emulation by oracle_pair): NCHW in, a tuple of NCHW
# out.  Disparities are judged on the UPDATE (output minus input disparity): the emulation stores a 300 px disparity on a 0.25 px grid,
# which would otherwise set the scale of the yardstick.
REFINER, GLOBAL = "refiner", "global_refiner"
MASK4, MASK1 = "upsample_mask_4x_refine", "upsample_mask_1x"
UP4_SCALE = 4.0                    # the x4 on the disparity that goes with the 1/4 -> 1/1 upsampling (s2m2.py:183)


def uniform16(shape, seed: int, lo: float, hi: float) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return round16(lo + (hi - lo) * torch.rand(*shape, generator=g))


def _xs(w: int) -> torch.Tensor:
    return torch.arange(w, dtype=torch.float32).reshape(1, 1, 1, w)


def occ_mask(occ: torch.Tensor, disp: torch.Tensor) -> torch.Tensor:
    """the loop epilogue of s2m2.py:179: no occlusion value where the match would lie left of the image"""
    return occ * (_xs(disp.shape[-1]) - disp >= 0)


def seeded_cv(sd: Mapping[str, torch.Tensor], c: int, h: int, w: int, seed: int) -> torch.Tensor:
    """the fp16 cost volume of O.disp_init on seeded tokens whose right view is the left one moved 8 tokens (a ridge at d = 8 over a
    background of chance matches) -> (1, h, w, w), values on the fp16 grid"""
    tok = peaked_pair((2, c, h, w), seed, 8)
    with torch.no_grad(), O.precision("fp16"):
        return O.ln_corr(tok, sd["disp_init.layer_norm.weight"], sd["disp_init.layer_norm.bias"]).contiguous()


def refine_inputs(sd: Mapping[str, torch.Tensor], c: int, h: int, w: int, far: bool, seed: int, masked_occ: bool = False):
    """(hidden, ctx, disp, conf, occ, cv) of one LocalRefiner iteration.  near: disparities uniform in [0, 16) px (fp16 quantum <= 2^-7);
    far: up to w - 1 (the lookups at the far end of the row and the taps outside it).  conf, occ uniform in (0, 1), all on the fp16 grid.
    masked_occ: occ as a previous iteration's epilogue leaves it (occ_mask)."""
    ctx = seeded((1, c, h, w), seed)
    hidden = round16(torch.tanh(ctx))
    disp = uniform16((1, 1, h, w), seed + 1, 0.0, float(w - 1) if far else 16.0)
    conf, occ = uniform16((1, 1, h, w), seed + 2, 0.0, 1.0), uniform16((1, 1, h, w), seed + 3, 0.0, 1.0)
    if masked_occ:
        occ = occ_mask(occ, disp)
    return hidden, ctx, disp, conf, occ, seeded_cv(sd, c, h, w, seed + 4)


def o_global_refiner(sd, ctx, disp, conf):
    """O.global_refiner + the positivity clamp of O._forward -> (disp_g - disp, the same without the clamp).  On seeded weights most
    of the low-confidence pixels get a negative disparity, which the clamp makes exact on every side: the unclamped update is what pins
    the module's arithmetic."""
    g = O.global_refiner(sd, GLOBAL, ctx, disp, conf)
    return g.clamp(min=0) - disp, g - disp


def o_ctx(sd, tr0, py0):
    """feat_fusion_layer -> ctx_feat -> tanh as in O._forward -> (ctx, hidden)"""
    fus = O.feature_fusion(sd, "feat_fusion_layer", tr0, py0)
    ctx = O._conv(sd, "ctx_feat.2", O._gelu(O._conv(sd, "ctx_feat.0", fus)))
    return ctx, O._q(torch.tanh(ctx))


def side_input(disp, conf, occ):
    """what the next iteration's LocalRefiner computes first from the state it is handed: (disp / 1e2, logit conf), (logit occ)"""
    return (torch.cat([O._q(disp / 1e2), O._q(torch.logit(conf, eps=1e-2))], 1), O._q(torch.logit(occ, eps=1e-2)))


def o_refine(sd, hidden, ctx, disp, conf, occ, cv, first: bool, want_side: bool):
    """one iteration of the refinement loop of O._forward (use_positivity): LocalRefiner, clamp, occlusion mask ->
    (hidden, disp update, conf, occ, corr1, corr2 [, side input (disp / 1e2, logit conf), side input (logit occ)]).  first: the
    iteration that gets DispInit's occ, which autocast holds in fp32 (occ_is_fp32 in the emulation)."""
    hn, d, c, o, (c1, c2) = O.local_refiner(sd, REFINER, hidden, ctx, disp, conf, occ, cv, occ_is_fp32=first and O._Prec.half)
    d = d.clamp(min=0)
    o = occ_mask(o, d)
    out = (hn, d - disp, c, o, c1, c2)
    return out + side_input(d, c, o) if want_side else out


OCC_OUTPUTS = (3, 7)               # o_refine outputs that carry the discontinuity occ * (x - disp >= 0)
MAX_MASKED = 0.01                  # at most this fraction of the pixels may be left out of the occ statistics (a condition on the case)


def occ_keep(disp_in: torch.Tensor, upd32: torch.Tensor, upd16e: torch.Tensor) -> torch.Tensor:
    """keep-mask of the occ outputs, from the oracle alone: the pixels whose x - disp (fp32) is further from the jump at 0 than
    MAX_RATIO x the emulation's largest disparity error of this case (closer, an admissible disparity error flips the mask)"""
    margin = MAX_RATIO * float((upd16e - upd32).abs().max())
    return (_xs(disp_in.shape[-1]) - (disp_in + upd32)).abs() > margin


def o_mask4x(sd, hidden, f2x):
    return (O.upsample_mask_4x(sd, MASK4, hidden, f2x),)


def o_mask1x(sd, disp_up, rgb, f2x):
    return (O.upsample_mask_1x(sd, MASK1, disp_up, rgb, f2x),)


def o_upsample4x(sd, disp, occ, conf, m4):
    """-> the three full-resolution maps and channel 0 of the image tensor (the disparity as UpsampleMask1x's conv reads it)"""
    d = O.upsample4x(O._q(disp * UP4_SCALE), m4)
    return d, O.upsample4x(occ, m4), O.upsample4x(conf, m4), O._q(d)


def o_upsample1x(sd, d_up, o_up, c_up, m1, output_upsample: bool = False):
    s = 2.0 if output_upsample else 1.0
    return s * O.upsample1x(d_up, m1, output_upsample), O.upsample1x(o_up, m1, output_upsample), O.upsample1x(c_up, m1, output_upsample)


def capture_refine(sd, img_left, f2_left, py0, tr, refine_iter: int) -> Dict[str, Tuple[torch.Tensor, ...]]:
    """the refinement half of O._forward (use_positivity) in fp32 from the trunk's outputs, with global_refiner, local_refiner,
    upsample_mask_* and upsample*x patched to record their tensor arguments -> {"refine:global_refiner", "refine:ctx", "refine:it<k>",
    "refine:mask4x", "refine:up4", "refine:mask1x", "refine:up1": inputs of the o_* function of that kind}"""
    got: Dict[str, Tuple[torch.Tensor, ...]] = {}
    calls = {"it": 0, "up4": 0, "up1": 0}

    def keep(key, *a):
        got.setdefault(key, tuple(t.clone() for t in a))

    real = {n: getattr(O, n) for n in ("global_refiner", "local_refiner", "upsample_mask_4x", "upsample_mask_1x", "upsample4x", "upsample1x")}

    def global_refiner(sd_, p, ctx, disp, conf):
        keep("refine:global_refiner", ctx, disp, conf)
        return real["global_refiner"](sd_, p, ctx, disp, conf)

    def local_refiner(sd_, p, hidden, ctx, disp, conf, occ, cv, occ_is_fp32=False):
        keep("refine:it%d" % calls["it"], hidden, ctx, disp, conf, occ, cv)
        calls["it"] += 1
        return real["local_refiner"](sd_, p, hidden, ctx, disp, conf, occ, cv, occ_is_fp32)

    def mask4(sd_, p, hidden, f2x):
        keep("refine:mask4x", hidden, f2x)
        return real["upsample_mask_4x"](sd_, p, hidden, f2x)

    def mask1(sd_, p, disp, rgb, f2x):
        keep("refine:mask1x", disp, rgb, f2x)
        return real["upsample_mask_1x"](sd_, p, disp, rgb, f2x)

    ups4, ups1 = [], []

    def up4(x, logits):
        ups4.append(x)
        return real["upsample4x"](x, logits)

    def up1(x, logits, output_upsample=False):
        ups1.append(x)
        return real["upsample1x"](x, logits, output_upsample)

    with contextlib.ExitStack() as st, torch.no_grad(), O.precision("fp32"):
        for name, fn in (("global_refiner", global_refiner), ("local_refiner", local_refiner), ("upsample_mask_4x", mask4),
                         ("upsample_mask_1x", mask1), ("upsample4x", up4), ("upsample1x", up1)):
            st.enter_context(patched(O, name, fn))
        B = img_left.shape[0]
        disp, conf, occ, cv, _, _ = O.disp_init(sd, tr, True)
        tr0 = tr[:B].contiguous()
        disp = O.global_refiner(sd, GLOBAL, tr0, disp, conf).clamp(min=0)
        keep("refine:ctx", tr0, py0)
        ctx, hidden = o_ctx(sd, tr0, py0)
        for _ in range(refine_iter):
            hidden, disp, conf, occ, _ = O.local_refiner(sd, REFINER, hidden, ctx, disp, conf, occ, cv)
            disp = disp.clamp(min=0)
            occ = occ_mask(occ, disp)
        m4 = O.upsample_mask_4x(sd, MASK4, hidden, f2_left)
        ups = [O.upsample4x(t, m4) for t in (disp * 4, occ, conf)]
        keep("refine:up4", disp, ups4[1], ups4[2], m4)
        m1 = O.upsample_mask_1x(sd, MASK1, ups[0], img_left, f2_left)
        for t in ups:
            O.upsample1x(t, m1)
        keep("refine:up1", *ups1, m1)
    return got
