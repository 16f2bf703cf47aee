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


def error_stats(y: torch.Tensor, y32: torch.Tensor) -> Dict[str, float]:
    e = (y.float() - y32.float()).abs().reshape(-1)
    over = e > ULPS * fp16_ulp(y32.float()).reshape(-1)
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


def judge(yh: torch.Tensor, y32: torch.Tensor, y16e: torch.Tensor, name: str = "") -> Verdict:
    """All three (n, h, w, c).  Passes iff yh is finite; median / p99 of |yh - y32| <= Q_RATIO x those of |y16e - y32| + floor; max <=
    MAX_RATIO x the emulation's max + floor; at most ULP_FRAC of the elements beyond ULPS fp16 ulps of y32.  The message of a failure
    names the (n, h, w, c) of the largest error and the error profile along w (tiles of 32 tokens) and c (groups of 16 channels)."""
    yh, y32, y16e = yh.detach().float().cpu(), y32.detach().float().cpu(), y16e.detach().float().cpu()
    if yh.shape != y32.shape or y16e.shape != y32.shape:
        raise AssertionError(f"{name}: shapes {tuple(yh.shape)} / {tuple(y32.shape)} / {tuple(y16e.shape)}")
    emu = error_stats(y16e, y32)
    if not bool(torch.isfinite(yh).all()):
        bad = (~torch.isfinite(yh)).nonzero()[0].tolist()
        return Verdict(False, f"{name}: {int((~torch.isfinite(yh)).sum())} non-finite elements, first at (n,h,w,c)={bad}", emu, emu)
    hip = error_stats(yh, y32)
    floor = FLOOR * float(y32.pow(2).mean().sqrt())
    fails = []
    for k in ("median", "p99"):
        if hip[k] > Q_RATIO * emu[k] + floor:
            fails.append(f"{k} {hip[k]:.3g} > {Q_RATIO} x {emu[k]:.3g} + {floor:.2g}")
    if hip["max"] > MAX_RATIO * emu["max"] + floor:
        fails.append(f"max {hip['max']:.3g} > {MAX_RATIO} x {emu['max']:.3g} + {floor:.2g}")
    if hip["ulp_frac"] > max(ULP_FRAC, emu["ulp_frac"]):
        fails.append(f"{hip['ulp_frac']:.3g} of the elements beyond {ULPS} fp16 ulps (emulation: {emu['ulp_frac']:.3g})")
    v = Verdict(not fails, "", hip, emu)
    if fails:
        err = (yh - y32).abs()
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


def capture_boundaries(sd: Mapping[str, torch.Tensor], x: torch.Tensor, ntr: int) -> Dict[str, Tuple[torch.Tensor, ...]]:
    """regime (a): the oracle's own fp32 inputs of every module of the trunk (CNN encoder, feature pyramid, transformers) on image
    tensor x (2B, 3, H, W) normalised to [-1, 1] -> {module prefix: its positional tensor arguments}."""
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
        f4, _ = O.cnn_encoder(sd, "cnn_backbone", x)
        z = O.unet(sd, "feat_pyramid", f4)
        for i in range(ntr):
            z = O.mrt(sd, f"transformer.uformer_list.{i}", *z)
    return got


def pick(t: torch.Tensor, rows: Optional[int]) -> torch.Tensor:
    """the first ``rows`` rows (full width) of an (n, c, h, w) tensor, or all of it"""
    return t if rows is None or rows >= t.shape[2] else t[:, :, :rows].contiguous()
