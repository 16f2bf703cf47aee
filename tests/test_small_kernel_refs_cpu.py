"""The comparators of tests/test_hip_small_kernels.py have teeth (CPU).

Every float64 reference (tests/small_kernel_refs.py) is run against the torch fp32 emulations of tests/fake_hip.py on the GPU tests' own
inputs and bounds (tests/small_kernel_cases.py) -- these must PASS -- and against small, deliberately wrong variants written here, each of
which must be REJECTED by the same comparator on the same inputs.  Where fake_hip.py has no emulation (image_pad), or differs from the
kernel's stated rounding points (the stem's hidden layer and the x2 logits of logit_up2 are held in the I/O dtype), a few lines of torch fp32
restate the operation.  S2M2_SMALL_KERNELS_MUTATIONS=<path> writes the rejection margins (profiles/r07/small_kernel_edges.txt).
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import small_kernel_cases as K
from fake_hip import make as _fake_hip

TABLE = []


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    path = os.environ.get("S2M2_SMALL_KERNELS_MUTATIONS")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(TABLE) + "\n")


class Emu:
    """the impl protocol of small_kernel_cases.evaluate on torch fp32 CPU ops; keyword flags switch ONE deliberate mistake on"""

    def __init__(self, **mut):
        self.mut = mut
        self.h = _fake_hip()

    def on(self, name):
        return bool(self.mut.get(name))

    def layernorm(self, x, wide_out):
        if not self.on("unbiased"):
            return [self.h.layernorm(x)]
        xf = x.float()
        return [((xf - xf.mean(-1, keepdim=True)) / torch.sqrt(xf.var(-1, unbiased=True, keepdim=True) + 1e-5)).to(x.dtype)]

    def groupnorm(self, x, G, gamma, beta):
        if self.on("yardstick"):                                       # torch's own F.group_norm (fake_hip.py)
            return [self.h.groupnorm_nhwc(x, G, gamma, beta)]
        # two-pass fp32 restatement: torch's CPU F.group_norm forms the variance from one-pass fp32 moments and misses the fixed fp32
        # tolerance on the replicas input by itself (sample 1 has mean / std = 6: 3.9e-5 against 3e-5, recorded in the table)
        N, H, W, C = x.shape
        xg = x.float().reshape(N, H * W, G, C // G)
        dims = (0, 1, 3) if self.on("shared_stats") else (1, 3)
        m, v = xg.mean(dims, keepdim=True), xg.var(dims, unbiased=self.on("unbiased"), keepdim=True)
        return [(((xg - m) / torch.sqrt(v + 1e-5)).reshape(N, H, W, C) * gamma + beta).to(x.dtype)]

    def convex_upsample(self, maps, logits, factor, scales, logit_up2):
        plain = not any(self.on(k) for k in ("zero_pad", "swap_n", "round_div", "softmax16"))
        if plain and not logit_up2:
            outs = [o[:, 0] for o in self.h.convex_upsample(maps, logits, factor, scales)]
            return outs + [outs[0].to(logits.dtype)]
        lg = logits[..., :16 if self.on("softmax16") else 9].float().permute(0, 3, 1, 2)
        if logit_up2:                                                  # the model holds the x2 logits in the activation dtype
            lg = F.interpolate(lg, scale_factor=2, mode="bilinear", align_corners=False).to(logits.dtype).float()
        wgt = lg.softmax(1)[:, :9]
        outs = []
        for m, s in zip(maps, scales):
            B, h, w = m.shape
            xp = F.pad(m[:, None], (1, 1, 1, 1), mode="constant" if self.on("zero_pad") else "replicate")
            offs = [(n % 3, n // 3) if self.on("swap_n") else (n // 3, n % 3) for n in range(9)]
            n9 = torch.cat([xp[:, :, dy:dy + h, dx:dx + w] for dy, dx in offs], 1)
            src = lambda n_out, n_in: (((torch.arange(n_out).float() / factor + 0.5).floor() if self.on("round_div") else
                                        (torch.arange(n_out) // factor).float()).long().clamp(max=n_in - 1))
            n9 = n9[:, :, src(h * factor, h)][:, :, :, src(w * factor, w)]
            outs.append((n9 * wgt).sum(1) * s)
        return outs + [outs[0].to(logits.dtype)]

    def resample2x(self, x, mode, strided):
        if mode == 1 and self.on("align_corners"):
            y = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
            return [y.permute(0, 2, 3, 1).to(x.dtype)]
        return [self.h.resample2x(x, mode)]

    def image_prep(self, img0, img1, dtype):
        return [self.h.image_prep(img0, img1, dtype)]

    def _logit_eps(self, local):
        return (1e-2 if local else 1e-1) if not self.on("swap_eps") else (1e-1 if local else 1e-2)

    def refine_prep(self, disp, conf, occ, mode, dtype):
        if not (self.on("thr_ge") or self.on("swap_eps")):
            return [self.h.refine_prep(disp, conf, occ, mode, dtype)]
        small = torch.zeros(disp.shape[0], disp.shape[2], disp.shape[3], 8, dtype=dtype)
        if mode == 0:
            mask = ((conf >= 0.2) if self.on("thr_ge") else (conf > 0.2)).float()
            small[..., 0] = (disp / 1e2 * mask)[:, 0]
            small[..., 1] = torch.logit(mask * conf, eps=self._logit_eps(False))[:, 0]
        else:
            small[..., 0] = (disp / 1e2)[:, 0]
            small[..., 1] = torch.logit(conf, eps=self._logit_eps(True))[:, 0]
            small[..., 2] = torch.logit(occ, eps=self._logit_eps(True))[:, 0]
        return [small]

    def global_update(self, upd, disp, conf, clamp0):
        if self.on("ignore_clamp0"):
            clamp0 = 0
        if not self.on("thr_ge"):
            return [self.h.global_update(upd, disp, conf, clamp0)]
        mask = (conf >= 0.2).float()
        d = mask * disp + (1 - mask) * (upd[..., 0].float().unsqueeze(1) * 1e2)
        return [d.clamp(min=0) if clamp0 else d]

    def refine_update(self, dco, disp, conf, occ, use_positivity, want_small):
        if not any(self.on(k) for k in ("strict_occ", "pos_always", "pos_never", "swap_ch", "swap_eps")):
            return list(self.h.refine_update(dco, disp, conf, occ, use_positivity, want_small))
        f = dco.float()
        c8, c9 = (9, 8) if self.on("swap_ch") else (8, 9)
        eps = self._logit_eps(True)
        d = disp + f[..., 0].unsqueeze(1)
        c = torch.sigmoid(f[..., c8].unsqueeze(1) + torch.logit(conf, eps=eps))
        o = torch.sigmoid(f[..., c9].unsqueeze(1) + torch.logit(occ, eps=eps))
        if (use_positivity or self.on("pos_always")) and not self.on("pos_never"):
            d = d.clamp(min=0)
        xs = torch.arange(d.shape[-1], dtype=torch.float32).reshape(1, 1, 1, -1)
        o = o * ((xs - d > 0) if self.on("strict_occ") else (xs - d >= 0))
        return [d, c, o] + ([self.h.refine_prep(d, c, o, 1, dco.dtype)] if want_small else [])

    def tanh(self, x):
        return [self.h.tanh(x.float()).to(x.dtype)]

    def stem_mlp(self, x8, w0, b0, w1, b1):
        if self.on("skip_row15"):                                      # the all-zero test of a column looks at rows 0..14 only
            w0 = w0 * (w0[:15].abs().sum(0, keepdim=True) > 0)
        h = F.gelu(F.linear(x8.float(), w0, b0)).to(x8.dtype).float()   # the hidden layer is held in the I/O dtype
        y = F.linear(h, w1, b1).to(x8.dtype)
        if self.on("skip_last_odd") and x8.shape[0] % 2:
            y[-1] = K.CANARY                                            # never written: the buffer's fill shows
        return [y]

    def image_pad(self, img, factor):
        H, W = img.shape[-2:]
        Hn, Wn = math.ceil(H / factor) * factor, math.ceil(W / factor) * factor
        ph, pw = Hn - H, Wn - W
        t, l = (ph - ph // 2, pw - pw // 2) if self.on("ceil_offset") else (ph // 2, pw // 2)
        x = F.pad(img.float(), (l, pw - l, t, ph - t), "constant", 0)
        down = F.adaptive_avg_pool2d(x, output_size=[H // factor, W // factor])
        out = F.interpolate(down, size=[Hn, Wn], mode="bilinear")
        out[:, :, t: t + H, l: l + W] = img.float()
        return [out]


@pytest.mark.parametrize("case", K.all_cases(), ids=lambda c: c.id)
def test_emulation_passes_at_the_gpu_tolerances(case):
    rows = K.evaluate(case, Emu())
    for r in rows:
        print(r.line())
    assert all(r.ratio <= 1 for r in rows), "\n".join(r.line() for r in rows)


@pytest.mark.parametrize("name", ["mean200-std0.5-C256", "mean30-std0.5-C256", "cancel-mean32-std2-1x40x40x128-G8"])
def test_yardstick_passes_the_derived_bounds(name):
    """torch's own fp32 F.layer_norm / F.group_norm is the yardstick of the two derived bounds: were it worse than the bound on one of these
    inputs, that input's mean / std would have to shrink until it passes with margin 2 (the bound does not grow).  It is not: the ratios
    go into the table."""
    cases = [c for c in K.all_cases() if c.name == name]
    assert cases
    for c in cases:
        for r in K.evaluate(c, Emu(yardstick=True)):
            TABLE.append(f"yardstick (torch fp32, CPU) {r.line()}")
            assert r.ratio <= 1, r.line()


# (operation, Emu flag, what is wrong)
MUTATIONS = [
    ("refine_prep", "thr_ge", "conf >= 0.2 in place of >"),
    ("global_update", "thr_ge", "conf >= 0.2 in place of >"),
    ("refine_update", "strict_occ", "x - d > 0 in place of >="),
    ("refine_prep", "swap_eps", "logit eps 1e-1 and 1e-2 exchanged"),
    ("refine_update", "swap_eps", "logit eps 1e-1 in place of 1e-2"),
    ("refine_update", "pos_always", "positivity clamp applied when use_positivity = 0"),
    ("refine_update", "pos_never", "positivity clamp dropped when use_positivity = 1"),
    ("global_update", "ignore_clamp0", "clamp0 ignored"),
    ("refine_update", "swap_ch", "channel 9 read for confidence and channel 8 for occlusion"),
    ("convex_upsample", "zero_pad", "zero padding in place of replicate padding in the 3 x 3 neighbourhood"),
    ("convex_upsample", "swap_n", "neighbour index n % 3 used for the row and n / 3 for the column"),
    ("convex_upsample", "round_div", "X / factor rounded instead of floored"),
    ("convex_upsample", "softmax16", "padding logits (channels 9-15) included in the softmax"),
    ("layernorm", "unbiased", "unbiased variance in LayerNorm"),
    ("groupnorm", "unbiased", "unbiased variance in GroupNorm"),
    ("groupnorm", "shared_stats", "GroupNorm statistics shared between the two samples of a batch"),
    ("stem_mlp", "skip_last_odd", "the last pixel of an odd npix left unwritten"),
    ("stem_mlp", "skip_row15", "a w0 column skipped when only its row-15 weight is non-zero"),
    ("image_pad", "ceil_offset", "hs = ceil in place of floor"),
    ("resample2x", "align_corners", "align_corners=True bilinear"),
]


@pytest.mark.parametrize("op,flag,what", MUTATIONS, ids=[f"{o}-{f}" for o, f, _ in MUTATIONS])
def test_wrong_variant_is_rejected(op, flag, what):
    rows = [r for c in K.cases_of(op) for r in K.evaluate(c, Emu(**{flag: True}))]
    bad = [r for r in rows if r.ratio > 1]
    worst = max(rows, key=lambda r: r.ratio)
    finite = max((r.ratio for r in rows if math.isfinite(r.ratio)), default=0.0)
    TABLE.append(f"mutation {op}: {what}: {'rejected' if bad else 'PASSED'} by {len(bad)} of {len(rows)} comparisons; worst error / bound "
                 f"{worst.ratio:.3g} ({worst.case.id} {worst.label}), worst finite {finite:.3g}")
    print(TABLE[-1])
    assert bad, f"{op}: '{what}' passes every case: the inputs are too weak"
