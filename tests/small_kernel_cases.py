"""Inputs, bounds and the one comparator of the small-kernel edge tests, shared by tests/test_hip_small_kernels.py (the HIP kernels through the
C ABI) and tests/test_small_kernel_refs_cpu.py (torch emulations and deliberately wrong variants): what rejects a wrong variant on the CPU is
literally what the GPU test runs.

A case names an operation, builds its inputs once on the CPU (already rounded to the I/O dtype) and lists (label, reference, bound) per output:
the reference is float64 (tests/small_kernel_refs.py) on the values the kernel reads, the bound an array or a scalar -- 0 means bit-exact.
evaluate(case, impl) calls impl.<op>(**args), which returns the outputs as CPU tensors, and gives one Row per output with the element of the
worst error / bound.  No element is masked.

Fixed tolerances (those of tests/test_hip_norm_upsample.py and tests/test_hip_utils.py, now against float64):
  LayerNorm 2e-5 / 2e-3, GroupNorm 3e-5 / 4e-3, upsampling 2e-5 * (max|ref| + 1), resample 1e-6 / 2e-3, point-wise stages 1e-5 / 2e-3
  (tanh and image_prep keep their tighter 1e-6 / 1e-3), stem 2e-5 / 4e-3, image_pad 2e-3.
Derived bounds, from the arithmetic of the kernels and nothing measured:
  high-mean LayerNorm  fixed + 16 * 2^-24 * max|x| * rstd_row (+ one output ulp in fp16): first-order rounding of a mean summed as C/16
                       sequential fp32 terms and four shuffle steps;
  high-mean GroupNorm  fixed + 0.5 * n_t * 2^-24 * (1 + (mean/std)^2) * |y|, n_t = 512 * C / nact the elements one thread adds in fp32 before
                       the fp64 atomic: the relative error E[x^2] can carry into E[x^2] - m^2.
"""
import functools

import numpy as np
import torch

import small_kernel_refs as R

TDT = {"float32": torch.float32, "float16": torch.float16}
SHORT = {"float32": "fp32", "float16": "fp16"}
DTYPES = ("float32", "float16")
CANARY = 7.0

TOL_LN = {"float32": 2e-5, "float16": 2e-3}
TOL_GN = {"float32": 3e-5, "float16": 4e-3}
TOL_RS = {"float32": 1e-6, "float16": 2e-3}
TOL_PW = {"float32": 1e-5, "float16": 2e-3}
TOL_TANH = {"float32": 1e-6, "float16": 1e-3}
TOL_PREP = {"float32": 1e-6, "float16": 1e-3}
TOL_STEM = {"float32": 2e-5, "float16": 4e-3}
TOL_PAD = 2e-3


def ulp(a, dtype):
    """spacing of dtype at |a| (normal range)"""
    a = np.abs(np.asarray(a, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14 if dtype == "float16" else 2.0 ** -126)))
    return 2.0 ** (e - (10 if dtype == "float16" else 23))


class Row:
    def __init__(self, case, label, err, bound, ratio):
        self.case, self.label, self.err, self.bound, self.ratio = case, label, err, bound, ratio

    def line(self):
        c = self.case
        return (f"{c.op:16s} {c.name:34s} {SHORT[c.dtype]}  {self.label:8s} max err {self.err:.3g}  bound {self.bound:.3g}  ratio "
                f"{self.ratio:.3g}  {'ok' if self.ratio <= 1 else 'FAIL'}")


class Case:
    def __init__(self, op, name, dtype, build):
        self.op, self.name, self.dtype, self._build = op, name, dtype, build
        self.id = f"{op}-{name}-{SHORT[dtype]}"

    @functools.lru_cache(maxsize=None)
    def built(self):
        """(args, checks): built once per process and shared; nothing may write into it"""
        return self._build()


def evaluate(case, impl):
    args, checks = case.built()
    outs = getattr(impl, case.op)(**args)
    rows = []
    for label, out, ref, bound in checks(outs):
        out = R.f64(out)
        assert out.shape == ref.shape, f"{case.id} {label}: shape {out.shape}, expected {ref.shape}"
        err = np.abs(out - ref)
        bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
        ratio = np.where(np.isfinite(err), ratio, np.inf)
        i = int(np.argmax(ratio)) if ratio.size else 0
        rows.append(Row(case, label, float(err.flat[i]), float(bound.flat[i]), float(ratio.flat[i])))
    return rows


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


# ------------------------------------------------------------------------------------------------------------------------------ LayerNorm
def _ln_case(name, dtype, rows, C, mean=1.5, std=3.0, const_row=None, wide_out=False, high_mean=False):
    def build():
        g = _gen(rows * 1000 + C)
        wide = (_randn(g, rows, 2 * C) * std + mean).to(TDT[dtype])
        if const_row is not None:
            wide[const_row] = 3.0
        x = wide[:, C:]                                                # strided rows: a channel slice of a wider tensor
        xd = R.f64(x)
        ref = R.layernorm(xd)
        bound = np.full(ref.shape, TOL_LN[dtype])
        if high_mean:
            rstd = 1.0 / np.sqrt(xd.var(-1, keepdims=True) + 1e-5)
            bound = bound + 16 * 2.0 ** -24 * np.abs(xd).max(-1, keepdims=True) * rstd
            if dtype == "float16":
                bound = bound + ulp(ref, dtype)
        if const_row is not None:
            bound[const_row] = 0.0                                      # every partial sum is exact: mean = 3, x - mean = 0
        return dict(x=x, wide_out=wide_out), lambda outs: [("y", outs[0], ref, bound)]
    return Case("layernorm", name, dtype, build)


def layernorm_cases():
    cs = []
    for dt in DTYPES:
        cs += [_ln_case("rows1-C128", dt, 1, 128),
               _ln_case("rows17-C128", dt, 17, 128),                  # the second block holds ONE live 16-lane group
               _ln_case("rows17-C768", dt, 17, 768),
               _ln_case("const-row-C128", dt, 3, 128, const_row=1),
               _ln_case("ystride-2C-C128", dt, 50, 128, wide_out=True)]
    cs.append(_ln_case("mean200-std0.5-C256", "float32", 17, 256, mean=200.0, std=0.5, high_mean=True))
    cs.append(_ln_case("mean30-std0.5-C256", "float16", 17, 256, mean=30.0, std=0.5, high_mean=True))
    return cs


# ------------------------------------------------------------------------------------------------------------------------------ GroupNorm
def gn_thread_terms(C, dtype):
    """n_t: fp32 additions of one thread of the statistics block (512 pixels) before its fp64 atomic"""
    P = C // (8 if dtype == "float16" else 4)
    return 512 * C // ((256 // P) * P)


def _gn_case(name, dtype, shape, kind="random"):
    N, H, W, C, G = shape

    def build():
        g = _gen(H * 131 + W * 7 + C + G)
        if kind == "two-samples":                                      # statistics that leak between samples or replicas show
            x = torch.stack([_randn(g, H, W, C) * 2 + 0.7, _randn(g, H, W, C) * 0.5 - 3.0])
        elif kind == "const":
            x = torch.full((N, H, W, C), 3.0)
        elif kind == "cancel":
            x = _randn(g, N, H, W, C) * 2 + 32.0
        else:
            x = _randn(g, N, H, W, C) * 2 + 0.7
        x = x.to(TDT[dtype])
        gamma = 1 + 0.1 * _randn(g, C)
        beta = 0.1 * _randn(g, C)
        xd = R.f64(x)
        ref = R.groupnorm_nhwc(xd, G, R.f64(gamma), R.f64(beta))
        bound = np.full(ref.shape, TOL_GN[dtype])
        if kind == "const":
            ref = np.broadcast_to(R.round_to(R.f64(beta), dtype), ref.shape).copy()     # mean = 3, var = 0 exactly: the output IS beta
            bound = 0.0
        if kind == "cancel":
            xg = xd.reshape(N, H * W, G, C // G)
            r2 = (xg.mean((1, 3), keepdims=True) ** 2 / xg.var((1, 3), keepdims=True))
            r2 = np.broadcast_to(r2, xg.shape).reshape(ref.shape)
            bound = bound + 0.5 * gn_thread_terms(C, dtype) * 2.0 ** -24 * (1 + r2) * np.abs(ref)
        return dict(x=x, G=G, gamma=gamma, beta=beta), lambda outs: [("y", outs[0], ref, bound)]
    return Case("groupnorm", name, dtype, build)


def groupnorm_cases():
    cs = []
    for dt in DTYPES:
        cs += [_gn_case("replicas-2x130x131x128-G8", dt, (2, 130, 131, 128, 8), "two-samples"),     # 34 statistics blocks per sample
               _gn_case("1x9x7x256-G32", dt, (1, 9, 7, 256, 32)),                                   # ppg = 1 (fp16) / 2 (fp32)
               _gn_case("1x9x7x64-G1", dt, (1, 9, 7, 64, 1)),
               _gn_case("1x6x6x512-G8", dt, (1, 6, 6, 512, 8)),                                     # P = 64 (fp16) / 128 (fp32)
               _gn_case("hw1-3x1x1x128-G8", dt, (3, 1, 1, 128, 8)),
               _gn_case("hw3-1x1x3x128-G8", dt, (1, 1, 3, 128, 8)),
               _gn_case("const3-1x8x8x128-G8", dt, (1, 8, 8, 128, 8), "const"),
               _gn_case("cancel-mean32-std2-1x40x40x128-G8", dt, (1, 40, 40, 128, 8), "cancel")]
    cs.append(_gn_case("cap-1x260x260x128-G8", "float16", (1, 260, 260, 128, 8)))                    # 67600 * 16 pieces > 4096 * 256
    cs.append(_gn_case("cap-1x182x182x128-G8", "float32", (1, 182, 182, 128, 8)))                    # 33124 * 32 pieces
    cs.append(_gn_case("ppg3-2x5x5x96-G4", "float16", (2, 5, 5, 96, 4)))                             # general (masked wave sum) path
    return cs


# ------------------------------------------------------------------------------------------------------------------------ convex upsample
def _up_case(name, dtype, B, hs, ws, factor, nmaps, up2=False, onehot=False):
    def build():
        g = _gen(B * 1000 + hs * 100 + ws * 10 + factor + nmaps)
        scales = [4.0, 1.0, 1.0][:nmaps]
        lh, lw = (hs, ws) if up2 else (hs * factor, ws * factor)
        big = torch.zeros(B, lh, lw, 32, dtype=TDT[dtype])
        big[..., :8] = CANARY * 3                                       # channels in front of the logits: never read
        lg = big[..., 8:32]                                            # logit rows of stride 32
        if onehot:                                                     # sample b: logit b sits 30 above the rest
            maps = [(1.0 + 0.37 * torch.arange(B * hs * ws, dtype=torch.float32)).reshape(B, hs, ws)]
            for b in range(B):
                lg[b, ..., b] = 30.0
        else:
            maps = [_randn(g, B, hs, ws) * s for s in (30.0, 1.0, 1.0)[:nmaps]]
            # multiples of 1/64 within +-7: exact in fp16, and every x2 bilinear combination of them (multiples of 1/1024) is exact in
            # fp32 -- the kernel and the float64 reference round the SAME number to the I/O dtype
            lg[..., :9] = ((_randn(g, B, lh, lw, 9) * 3).clamp(-7, 7) * 64).round() / 64
        lg[..., 9:16] = 50.0                                           # padding channels must be ignored
        md = [R.f64(m) for m in maps]
        refs = R.convex_upsample(md, R.f64(lg), factor, scales, up2, dtype)

        def checks(outs):
            rows = []
            for k in range(nmaps):
                if onehot:
                    n9 = R.neigh9(md[k]).repeat(factor, 2).repeat(factor, 3)
                    exact = np.stack([n9[b, b] for b in range(B)]) * scales[k]
                    rows.append((f"map{k}", outs[k], exact, 2 * ulp(exact, "float32")))      # the other eight weights total < 1e-12
                else:
                    rows.append((f"map{k}", outs[k], refs[k], 2e-5 * (np.abs(refs[k]).max() + 1)))
            # chan_out: the SAME map 0 the launch wrote, rounded once to the I/O dtype
            rows.append(("chan", outs[nmaps], R.f64(torch.as_tensor(outs[0]).to(TDT[dtype])), 0.0))
            return rows
        return dict(maps=maps, logits=lg, factor=factor, scales=scales, logit_up2=up2), checks
    return Case("convex_upsample", name, dtype, build)


def convex_upsample_cases():
    cs = []
    for dt in DTYPES:
        cs += [_up_case("1x1x1-f4-3maps", dt, 1, 1, 1, 4, 3),
               _up_case("1x1x7-f4-2maps", dt, 1, 1, 7, 4, 2),
               _up_case("2x5x1-f1-1map", dt, 2, 5, 1, 1, 1),
               _up_case("1x3x5-f2-3maps", dt, 1, 3, 5, 2, 3),
               _up_case("1x3x5-f2-up2-2maps", dt, 1, 3, 5, 2, 2, up2=True),
               _up_case("1x1x6-f2-up2-1map", dt, 1, 1, 6, 2, 1, up2=True),
               _up_case("onehot-9x3x5-f2", dt, 9, 3, 5, 2, 1, onehot=True)]
    return cs


# ------------------------------------------------------------------------------------------------------------------------------ resample2x
def _rs_case(name, dtype, shape, mode, strided=False, exact=False):
    N, H, W, C = shape

    def build():
        g = _gen(H * 100 + W * 10 + C + mode)
        if strided:
            x = _randn(g, N, H, W, 256).to(TDT[dtype])[..., 64:64 + C]
        else:
            x = _randn(g, N, H, W, C).to(TDT[dtype])
        ref = R.resample2x(R.f64(x), mode)
        return dict(x=x, mode=mode, strided=strided), lambda outs: [("y", outs[0], ref, 0.0 if exact else TOL_RS[dtype])]
    return Case("resample2x", name, dtype, build)


def resample2x_cases():
    cs = []
    for dt in DTYPES:
        cs += [_rs_case("bilinear-1x1x1x8", dt, (1, 1, 1, 8), 1, exact=True),      # all four outputs equal the input
               _rs_case("bilinear-1x1x5x8", dt, (1, 1, 5, 8), 1),
               _rs_case("bilinear-1x5x1x16", dt, (1, 5, 1, 16), 1),
               _rs_case("bilinear-2x3x7x192", dt, (2, 3, 7, 192), 1),
               _rs_case("pool-1x2x2x8", dt, (1, 2, 2, 8), 0),
               _rs_case("pool-2x6x10x384", dt, (2, 6, 10, 384), 0),
               _rs_case("bilinear-strided-1x4x6x128", dt, (1, 4, 6, 128), 1, strided=True),
               _rs_case("pool-strided-1x4x6x128", dt, (1, 4, 6, 128), 0, strided=True)]
    return cs


# ------------------------------------------------------------------------------------------------------------------------------ image_prep
IMG_DT = {"f32": torch.float32, "f16": torch.float16, "u8": torch.uint8}


def _prep_case(name, dtype, img, B, H, W, kind="random"):
    def build():
        g = _gen(B * 100 + H * 10 + W)
        if kind == "extremes":                                         # planes of all 0 and all 255: exactly -1 and +1
            a = torch.zeros(B, 3, H, W)
            a[:, 1] = 255.0
            b = 255.0 - a
        else:
            a = torch.randint(0, 256, (B, 3, H, W), generator=g).float()
            b = torch.randint(0, 256, (B, 3, H, W), generator=g).float()
        a, b = a.to(IMG_DT[img]), b.to(IMG_DT[img])
        ref = R.image_prep(R.f64(a), R.f64(b))
        bound = np.zeros(ref.shape)                                     # channels 0, 4..7: exact zeros
        bound[..., 1:4] = 0.0 if kind == "extremes" else TOL_PREP[dtype]
        return dict(img0=a, img1=b, dtype=TDT[dtype]), lambda outs: [("x8", outs[0], ref, bound)]
    return Case("image_prep", name, dtype, build)


def image_prep_cases():
    cs = []
    for dt in DTYPES:
        cs += [_prep_case("f16img-2x3x5x7", dt, "f16", 2, 5, 7),
               _prep_case("f16img-1x3x1x1", dt, "f16", 1, 1, 1),
               _prep_case("u8img-1x3x1x1", dt, "u8", 1, 1, 1)]
        cs += [_prep_case(f"{k}img-extremes-1x3x3x5", dt, k, 1, 3, 5, "extremes") for k in IMG_DT]
    return cs


# --------------------------------------------------------------------------------------- refine_prep / global_update / refine_update
def _grid_maps(B=2, h=3, w=37):
    """hand-built: every threshold, clamp and sign edge of the three kernels at known pixels"""
    n = B * h * w
    i = np.arange(n)
    col = (i % w).astype(np.float64)
    f02 = np.float32(0.2)
    levels = np.array([0.0, 0.01, f02, np.nextafter(f02, np.float32(1)), 0.5, 0.99, 1.0], dtype=np.float32)
    conf = levels[i % 7]
    occ = levels[(3 * i + 2) % 7]
    # disp + delta lands on: the column (x - d = 0: kept), column + 0.5 (masked), column - 0.5, negative, well inside, zero
    kind = (i // 7) % 6
    target = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [col, col + 0.5, col - 0.5, -1.5 - (i % 3), col - 3.0], 0.0)
    delta = np.array([0.0, 0.5, -0.5, 1.0, -2.0, 3.5])[(i // 42 + i) % 6]
    disp = (target - delta).astype(np.float32)                                     # integers and halves: disp + delta is exact in fp32
    lvl = np.array([0.0, 1.0, -1.0, 30.0, -30.0])
    d8, d9 = lvl[i % 5], lvl[(2 * i + 1) % 5]
    upd0 = np.array([0.25, -0.5, 1.0, -0.125, 0.75])[(i // 7 + i) % 5]              # fp16-exact; |upd * 100| < 128
    sh = (B, 1, h, w)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(sh)
    return t(disp), t(conf), t(occ), delta.reshape(B, h, w), d8.reshape(B, h, w), d9.reshape(B, h, w), upd0.reshape(B, h, w)


def _random_maps(g, B=1, h=5, w=257):
    """random, on grids that keep disp + delta exact (multiples of 1/8 and 1/16): a block boundary falls mid-row"""
    sh = (B, 1, h, w)
    disp = torch.randint(-16, 320, sh, generator=g).float() / 8
    conf, occ = torch.rand(sh, generator=g), torch.rand(sh, generator=g)
    delta = (torch.randint(-64, 65, (B, h, w), generator=g).float() / 16).numpy()
    d8, d9 = _randn(g, B, h, w).numpy(), _randn(g, B, h, w).numpy()
    upd0 = (_randn(g, B, h, w) * 0.4).clamp(-1.2, 1.2).numpy()
    return disp, conf, occ, delta, d8, d9, upd0


def _pw_maps(kind):
    return _grid_maps() if kind == "grid" else _random_maps(_gen(257))


def _upd_tensor(upd0, dtype, g):
    B, h, w = upd0.shape
    big = _randn(g, B, h, w, 24).to(TDT[dtype])
    big[..., 8] = torch.from_numpy(upd0).to(TDT[dtype])
    return big[..., 8:16]                                              # upd: channels 8:16 of a 24-wide tensor


def _dco_tensor(delta, d8, d9, dtype, g):
    B, h, w = delta.shape
    big = _randn(g, B, h, w, 32).to(TDT[dtype])
    for c, a in ((0, delta), (8, d8), (9, d9)):
        big[..., 16 + c] = torch.from_numpy(a).to(TDT[dtype])
    return big[..., 16:32]                                             # dco: channels 16:32 of a 32-wide tensor


def _m(t):
    return R.f64(t)[:, 0]


def _rp_case(kind, dtype, mode):
    def build():
        disp, conf, occ = _pw_maps(kind)[:3]
        ref = R.refine_prep(_m(disp), _m(conf), _m(occ), mode)
        bound = np.zeros(ref.shape)
        bound[..., :3 if mode else 2] = TOL_PW[dtype]
        return dict(disp=disp, conf=conf, occ=occ if mode else None, mode=mode, dtype=TDT[dtype]), \
            lambda outs: [("small", outs[0], ref, bound)]
    return Case("refine_prep", f"{kind}-mode{mode}", dtype, build)


def _gu_case(kind, dtype, clamp0):
    def build():
        disp, conf, _, _, _, _, upd0 = _pw_maps(kind)
        upd = _upd_tensor(upd0, dtype, _gen(11))
        ref = R.global_update(R.f64(upd[..., 0]), _m(disp), _m(conf), clamp0)[:, None]
        return dict(upd=upd, disp=disp, conf=conf, clamp0=clamp0), lambda outs: [("disp", outs[0], ref, TOL_PW["float32"])]
    return Case("global_update", f"{kind}-clamp{clamp0}", dtype, build)


def _ru_case(kind, dtype, use_pos, want_small):
    def build():
        disp, conf, occ, delta, d8, d9, _ = _pw_maps(kind)
        dco = _dco_tensor(delta, d8, d9, dtype, _gen(13))
        rd, rc, ro = (a[:, None] for a in R.refine_update(R.f64(dco), _m(disp), _m(conf), _m(occ), use_pos))

        def checks(outs):
            rows = [("disp", outs[0], rd, TOL_PW["float32"]), ("conf", outs[1], rc, TOL_PW["float32"]), ("occ", outs[2], ro, TOL_PW["float32"])]
            if want_small:                                             # refine_prep(mode 1) of the maps this launch wrote
                sref = R.refine_prep(_m(outs[0]), _m(outs[1]), _m(outs[2]), 1)
                sb = np.zeros(sref.shape)
                sb[..., :3] = TOL_PW[dtype]
                rows.append(("small", outs[3], sref, sb))
            return rows
        return dict(dco=dco, disp=disp, conf=conf, occ=occ, use_positivity=use_pos, want_small=want_small), checks
    return Case("refine_update", f"{kind}-pos{use_pos}-small{want_small}", dtype, build)


def refine_prep_cases():
    return [_rp_case(k, dt, m) for dt in DTYPES for k in ("grid", "random") for m in (0, 1)]


def global_update_cases():
    return [_gu_case("grid", dt, c) for dt in DTYPES for c in (0, 1)] + [_gu_case("random", dt, 1) for dt in DTYPES]


def refine_update_cases():
    return [_ru_case("grid", dt, p, s) for dt in DTYPES for p in (0, 1) for s in (0, 1)] + [_ru_case("random", dt, 1, 1) for dt in DTYPES]


# ------------------------------------------------------------------------------------------------------------------------------------ tanh
def _tanh_case(dtype, n):
    def build():
        x = _randn(_gen(n), n) * 3
        x[:8] = torch.tensor([0.0, -0.0, 12.0, -12.0, 2.0 ** -24, -2.0 ** -24, 0.5, -20.0])       # 2^-24: the smallest fp16 subnormal
        x = x.to(TDT[dtype])
        xd = R.f64(x)
        ref = R.tanh(xd)
        bound = np.full(ref.shape, TOL_TANH[dtype])
        if dtype == "float16":
            ref = np.where(np.abs(xd) >= 12, np.sign(xd), ref)          # |x| >= 12: exactly +-1 (1 - tanh(12) = 7.6e-11)
            bound[np.abs(xd) >= 12] = 0.0
        return dict(x=x), lambda outs: [("y", outs[0], ref, bound)]
    return Case("tanh", f"n{n}", dtype, build)


def tanh_cases():
    return [_tanh_case(dt, n) for dt in DTYPES for n in (8, 8 * 257)]


# -------------------------------------------------------------------------------------------------------------------------------- stem_mlp
STEM_W0 = ("dense", "negzero-col", "row15-only-col")


def stem_inputs(dtype, npix, w0_kind):
    g = _gen(npix)
    x8 = (torch.rand(npix, 8, generator=g) * 2 - 1).to(TDT[dtype])
    x8[x8 == 0] = 0.5                                                   # all 8 channels non-zero
    w0 = _randn(g, 16, 8) * (3.0 / 8.0) ** 0.5                          # the hidden layer keeps the spread of the 3-plane stem
    if w0_kind == "negzero-col":
        w0[:, 5] = -0.0
    elif w0_kind == "row15-only-col":
        w0[:, 2] = 0.0
        w0[15, 2] = 1.5
    w1 = _randn(g, 16, 16) / 4
    b0, b1 = _randn(g, 16), _randn(g, 16)
    return x8, w0, b0, w1, b1


def _stem_case(dtype, npix, w0_kind):
    def build():
        x8, w0, b0, w1, b1 = stem_inputs(dtype, npix, w0_kind)
        ref = R.stem_mlp(R.f64(x8), R.f64(w0), R.f64(b0), R.f64(w1), R.f64(b1), dtype)
        return dict(x8=x8, w0=w0, b0=b0, w1=w1, b1=b1), lambda outs: [("y", outs[0], ref, TOL_STEM[dtype])]
    return Case("stem_mlp", f"npix{npix}-{w0_kind}", dtype, build)


def stem_mlp_cases():
    return [_stem_case(dt, n, k) for dt in DTYPES for n in (1, 513, 1961) for k in STEM_W0]


# ------------------------------------------------------------------------------------------------------------------------------- image_pad
def _pad_case(img, shape, factor):
    def build():
        x = torch.randint(0, 256, shape, generator=_gen(shape[2] * 100 + shape[3])).float().to(IMG_DT[img])
        ref = R.image_pad(R.f64(x), factor)
        return dict(img=x, factor=factor), lambda outs: [("out", outs[0], ref, TOL_PAD)]
    return Case("image_pad", f"{img}img-{'x'.join(map(str, shape))}-f{factor}", "float32", build)


def image_pad_cases():
    shapes = [((1, 3, 33, 40), 32), ((1, 1, 32, 63), 32), ((2, 3, 50, 70), 16), ((5, 1, 40, 33), 32)]   # the first two and the last: ONE bin
    return [_pad_case(k, s, f) for k in IMG_DT for s, f in shapes]


ALL = {"layernorm": layernorm_cases, "groupnorm": groupnorm_cases, "convex_upsample": convex_upsample_cases, "resample2x": resample2x_cases,
       "image_prep": image_prep_cases, "refine_prep": refine_prep_cases, "global_update": global_update_cases,
       "refine_update": refine_update_cases, "tanh": tanh_cases, "stem_mlp": stem_mlp_cases, "image_pad": image_pad_cases}


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(c for op in ALL for c in ALL[op]())


def cases_of(op):
    return [c for c in all_cases() if c.op == op]
