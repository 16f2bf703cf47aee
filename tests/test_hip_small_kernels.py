"""Edge and grid-scale parity of the small kernels through the C ABI: K6 (norm.hip: layernorm_rows, groupnorm stats / apply), K7 (upsample.hip:
convex_upsample, resample2x) and K8 with image_pad (pointwise.hip) against float64 CPU references (tests/small_kernel_refs.py).

The cases, their inputs and bounds are in tests/small_kernel_cases.py; tests/test_small_kernel_refs_cpu.py shows on the CPU that the same
comparator on the same inputs rejects twenty one-line mistakes.  What each group of cases reaches that no earlier test did:
  groupnorm        replicas 2..31 of the fp64 statistics and their per-sample stride (34 blocks per sample, two samples of different
                   statistics); the 4096-block cap of the apply kernel and its grid-stride trip; G = 32, 1, 4 (ppg = 1, 2, 3, 8, 16; P = 64,
                   128; the masked-wave-sum path); HW = 1, 3; a constant input (var clamped at 0: the output IS beta, bit for bit);
                   E[x^2] - m^2 under cancellation (mean / std = 16); a workspace that is dirty on entry, twice
  layernorm        rows = 1; a block whose last 16-lane group is the only live one; y_stride != C; |mean| >> std; a constant row
  convex_upsample  hs = 1, ws = 1 (both clamps on one index); nmaps 1, 2, 3; factor 2 without logit_up2; logit rows of stride 32; chan_out
                   into channel 0 of an 8-channel tensor; a one-hot mask per neighbour (index order, replicate padding: exact)
  resample2x       H = 1, W = 1; C = 8 .. 384; x_stride != C and y_stride != C
  image_prep       the fp16 image type; one pixel; 0 and 255 give exactly -1 and +1
  refine_prep, global_update, refine_update
                   the strict and non-strict edges (conf > 0.2f at 0.2f and its successor, x - d >= 0 at 0 and +-0.5, the logit clamps at 0
                   and 1); use_positivity 0 / 1, clamp0 0 / 1, small_next on / off; upd_stride 24, dco_stride 32; a block boundary mid-row
  tanh             0, -0.0, +-12 (exactly +-1 in fp16), an fp16 subnormal; one piece and 257 pieces
  stem_mlp         odd pixel counts (the last thread's second store), one pixel, a dense w0, a -0.0 column, a column whose only non-zero
                   is w0[15, k]
  image_pad        a single bin (Ho = Wo = 1), factor 16, the fp16 image type
Every output that is a slice or has a tail is pre-filled with a canary (7.0) that must be bit-unchanged afterwards.
Measured error / bound of every case: profiles/r07/small_kernel_edges.txt (S2M2_SMALL_KERNELS_TABLE=<path> writes the rows).
"""
import os

import pytest
import torch
import torch.nn.functional as F

import small_kernel_cases as K
import small_kernel_refs as R

pytestmark = pytest.mark.gpu

TABLE = []
DT = {torch.float32: 0, torch.float16: 1}
IMG = {torch.float32: 0, torch.float16: 1, torch.uint8: 2}


@pytest.fixture(scope="module")
def lib():
    from s2m2_amd import hip as h
    return h.load()


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    path = os.environ.get("S2M2_SMALL_KERNELS_TABLE")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(TABLE) + "\n")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(lib, rc, what):
    assert rc == 0, f"{what}: {lib.s2m2_last_error().decode()}"
    torch.cuda.synchronize()


def _canary(t, what):
    assert bool((t == K.CANARY).all()), f"{what}: the canary was overwritten"


def _dev_view(view):
    """a channel slice view[..., a:b] of a wider CPU tensor -> the same slice of a device copy of the WHOLE tensor"""
    base = view._base if view._base is not None else view
    d = base.cuda()
    return d.as_strided(view.shape, view.stride(), view.storage_offset())


class Gpu:
    """the impl protocol of small_kernel_cases.evaluate on the HIP kernels: the s2m2_amd.hip wrappers where they can express the case, the
    raw entry points for output strides, tails and canaries"""

    def __init__(self, lib):
        from s2m2_amd import hip
        self.lib, self.hip = lib, hip

    def layernorm(self, x, wide_out):
        xd = _dev_view(x)
        if not wide_out:
            return [self.hip.layernorm(xd).cpu()]
        rows, C = x.shape
        wide = torch.full((rows, 2 * C), K.CANARY, device="cuda", dtype=x.dtype)
        y = wide[:, C:]
        _ok(self.lib, self.lib.s2m2_layernorm(xd.data_ptr(), y.data_ptr(), rows, C, xd.stride(0), 2 * C, DT[x.dtype], _stream()), "layernorm")
        _canary(wide[:, :C], "layernorm y_stride = 2C")
        return [y.cpu()]

    def groupnorm(self, x, G, gamma, beta):
        return [self.hip.groupnorm_nhwc(x.cuda(), G, gamma.cuda(), beta.cuda()).cpu()]

    def convex_upsample(self, maps, logits, factor, scales, logit_up2):
        lg = _dev_view(logits)
        B, hs, ws = maps[0].shape
        Ho, Wo = hs * factor, ws * factor
        x8 = torch.full((B, Ho, Wo, 8), K.CANARY, device="cuda", dtype=logits.dtype)
        outs = self.hip.convex_upsample([m.cuda() for m in maps], lg, factor, scales=scales, logit_up2=logit_up2, chan_out=x8[..., 0])
        torch.cuda.synchronize()
        _canary(x8[..., 1:], "convex_upsample chan_out, channels 1..7")
        return [o[:, 0].cpu() for o in outs] + [x8[..., 0].cpu()]

    def resample2x(self, x, mode, strided):
        xd = _dev_view(x)
        if not strided:
            return [self.hip.resample2x(xd, mode).cpu()]
        N, H, W, C = x.shape
        Ho, Wo = (H // 2, W // 2) if mode == 0 else (2 * H, 2 * W)
        wide = torch.full((N, Ho, Wo, C + 16), K.CANARY, device="cuda", dtype=x.dtype)
        y = wide[..., 8:8 + C]
        _ok(self.lib, self.lib.s2m2_resample2x(xd.data_ptr(), y.data_ptr(), N, H, W, C, xd.stride(2), C + 16, mode, DT[x.dtype], _stream()),
            "resample2x")
        _canary(wide[..., :8], "resample2x y slice, channels in front")
        _canary(wide[..., 8 + C:], "resample2x y slice, channels behind")
        return [y.cpu()]

    def image_prep(self, img0, img1, dtype):
        B, _, H, W = img0.shape
        n = 2 * B * H * W * 8
        buf = torch.full((n + 32,), K.CANARY, device="cuda", dtype=dtype)
        a, b = img0.cuda(), img1.cuda()
        _ok(self.lib, self.lib.s2m2_image_prep(a.data_ptr(), b.data_ptr(), buf.data_ptr(), B, H, W, IMG[img0.dtype], DT[dtype], _stream()),
            "image_prep")
        _canary(buf[n:], "image_prep tail")
        return [buf[:n].reshape(2 * B, H, W, 8).cpu()]

    def refine_prep(self, disp, conf, occ, mode, dtype):
        n = disp.numel()
        buf = torch.full((n * 8 + 32,), K.CANARY, device="cuda", dtype=dtype)
        d, c, o = disp.cuda(), conf.cuda(), occ.cuda() if occ is not None else None
        _ok(self.lib, self.lib.s2m2_refine_prep(d.data_ptr(), c.data_ptr(), o.data_ptr() if o is not None else None, buf.data_ptr(), n, mode,
                                                 DT[dtype], _stream()), "refine_prep")
        _canary(buf[n * 8:], "refine_prep tail")
        return [buf[:n * 8].reshape(disp.shape[0], disp.shape[2], disp.shape[3], 8).cpu()]

    def global_update(self, upd, disp, conf, clamp0):
        u = _dev_view(upd)
        n = disp.numel()
        buf = torch.full((n + 32,), K.CANARY, device="cuda")
        d, c = disp.cuda(), conf.cuda()
        _ok(self.lib, self.lib.s2m2_global_update(u.data_ptr(), u.stride(2), d.data_ptr(), c.data_ptr(), buf.data_ptr(), n, int(clamp0),
                                                   DT[upd.dtype], _stream()), "global_update")
        _canary(buf[n:], "global_update tail")
        return [buf[:n].reshape(disp.shape).cpu()]

    def refine_update(self, dco, disp, conf, occ, use_positivity, want_small):
        r = _dev_view(dco)
        n = disp.numel()
        B, _, h, w = disp.shape
        maps = torch.full((3, n + 32), K.CANARY, device="cuda")
        small = torch.full((n * 8 + 32,), K.CANARY, device="cuda", dtype=dco.dtype)
        d, c, o = disp.cuda(), conf.cuda(), occ.cuda()
        _ok(self.lib, self.lib.s2m2_refine_update_to(r.data_ptr(), r.stride(2), d.data_ptr(), c.data_ptr(), o.data_ptr(), maps[0].data_ptr(),
                                                      maps[1].data_ptr(), maps[2].data_ptr(), small.data_ptr() if want_small else None, n, w,
                                                      int(use_positivity), DT[dco.dtype], _stream()), "refine_update_to")
        _canary(maps[:, n:], "refine_update tails")
        _canary(small[n * 8:] if want_small else small, "refine_update small_next")
        outs = [maps[k, :n].reshape(disp.shape).cpu() for k in range(3)]
        # the in-place entry point is the same kernel with the outputs aliased to the inputs
        _ok(self.lib, self.lib.s2m2_refine_update(r.data_ptr(), r.stride(2), d.data_ptr(), c.data_ptr(), o.data_ptr(), n, w, int(use_positivity),
                                                   DT[dco.dtype], _stream()), "refine_update")
        for a, b in zip((d, c, o), outs):
            assert torch.equal(a.cpu(), b), "refine_update in place differs from refine_update_to"
        return outs + ([small[:n * 8].reshape(B, h, w, 8).cpu()] if want_small else [])

    def tanh(self, x):
        n = x.numel()
        buf = torch.full((n + 32,), K.CANARY, device="cuda", dtype=x.dtype)
        xd = x.cuda()
        _ok(self.lib, self.lib.s2m2_tanh(xd.data_ptr(), buf.data_ptr(), n, DT[x.dtype], _stream()), "tanh")
        _canary(buf[n:], "tanh tail")
        return [buf[:n].cpu()]

    def stem_mlp(self, x8, w0, b0, w1, b1):
        return [self.stem_raw(x8, w0, b0, w1, b1).cpu()]

    def stem_raw(self, x8, w0, b0, w1, b1):
        npix = x8.shape[0]
        buf = torch.full((npix + 4, 16), K.CANARY, device="cuda", dtype=x8.dtype)          # a 4-pixel canary tail
        t = [a.cuda().contiguous() for a in (x8, w0, b0, w1, b1)]
        _ok(self.lib, self.lib.s2m2_stem_mlp(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                                              buf.data_ptr(), npix, DT[x8.dtype], _stream()), "stem_mlp")
        _canary(buf[npix:], "stem_mlp tail (the pixel behind an odd count)")
        return buf[:npix]

    def image_pad(self, img, factor):
        B, C, H, W = img.shape
        Hn, Wn = -(-H // factor) * factor, -(-W // factor) * factor
        nb, n = B * C * (H // factor) * (W // factor), B * C * Hn * Wn
        pooled = torch.full((nb + 32,), K.CANARY, device="cuda")
        out = torch.full((n + 32,), K.CANARY, device="cuda")
        x = img.cuda()
        _ok(self.lib, self.lib.s2m2_image_pad(x.data_ptr(), pooled.data_ptr(), out.data_ptr(), B, C, H, W, factor, IMG[img.dtype], _stream()),
            "image_pad")
        _canary(pooled[nb:], "image_pad pooled tail")
        _canary(out[n:], "image_pad tail")
        return [out[:n].reshape(B, C, Hn, Wn).cpu()]


@pytest.mark.parametrize("case", K.all_cases(), ids=lambda c: c.id)
def test_small_kernel(lib, case):
    rows = K.evaluate(case, Gpu(lib))
    for r in rows:
        TABLE.append(r.line())
        print(r.line())
    assert all(r.ratio <= 1 for r in rows), "\n".join(r.line() for r in rows)


class _Yardstick:
    """torch's own fp32 kernels on the device, on the same inputs: the yardstick of the two derived bounds"""

    def layernorm(self, x, wide_out):
        return [F.layer_norm(x.cuda().float(), (x.shape[-1],)).cpu()]

    def groupnorm(self, x, G, gamma, beta):
        return [F.group_norm(x.cuda().float().permute(0, 3, 1, 2), G, gamma.cuda(), beta.cuda()).permute(0, 2, 3, 1).cpu()]


@pytest.mark.parametrize("name", ["mean200-std0.5-C256", "mean30-std0.5-C256", "cancel-mean32-std2-1x40x40x128-G8",
                                  "replicas-2x130x131x128-G8"])
def test_yardstick_passes_the_bounds(name):
    """were torch's fp32 F.layer_norm / F.group_norm worse than the bound on a high-mean input, the input's mean / std would have to shrink"""
    for c in [c for c in K.all_cases() if c.name == name]:
        for r in K.evaluate(c, _Yardstick()):
            TABLE.append(f"yardstick (torch fp32 on the device, unrounded output) {r.line()}")
            print(TABLE[-1])
            assert r.ratio <= 1, r.line()


@pytest.mark.parametrize("dtype", K.DTYPES)
def test_groupnorm_dirty_workspace(lib, dtype):
    """the header promises that the statistics workspace is zeroed inside: a raw call on a workspace full of 1e300, and a second one on
    what the first left behind, both give the result of a clean call"""
    case = next(c for c in K.cases_of("groupnorm") if c.name == "hw3-1x1x3x128-G8" and c.dtype == dtype)
    big = next(c for c in K.cases_of("groupnorm") if c.name == "replicas-2x130x131x128-G8" and c.dtype == dtype)
    for cs in (case, big):
        args, checks = cs.built()
        x, gamma, beta = args["x"].cuda(), args["gamma"].cuda(), args["beta"].cuda()
        N, H, W, C = x.shape
        nws = lib.s2m2_groupnorm_workspace_bytes(N, args["G"]) // 8
        ws = torch.full((nws + 4,), 1e300, device="cuda", dtype=torch.float64)
        for trip in range(2):
            y = torch.full((x.numel() + 32,), K.CANARY, device="cuda", dtype=x.dtype)
            _ok(lib, lib.s2m2_groupnorm_nhwc(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ws.data_ptr(), N, H * W, C,
                                             args["G"], 1e-5, DT[x.dtype], _stream()), "groupnorm_nhwc")
            _canary(y[x.numel():], "groupnorm tail")
            assert bool((ws[nws:] == 1e300).all()), "groupnorm wrote behind its workspace"
            (label, out, ref, bound), = checks([y[:x.numel()].reshape(x.shape).cpu()])
            err = abs(R.f64(out) - ref)
            ratio = float((err / bound).max())
            TABLE.append(f"groupnorm        dirty-workspace trip {trip} {cs.name} {K.SHORT[dtype]}  worst error / bound {ratio:.3g}")
            assert ratio <= 1, TABLE[-1]


@pytest.mark.parametrize("dtype", K.DTYPES)
@pytest.mark.parametrize("npix", [1, 513, 1961])
def test_stem_negative_zero_column_is_bit_identical(lib, dtype, npix):
    """a column of -0.0 weights is skipped like a column of +0.0 (the wave-uniform test shifts the sign bit out)"""
    x8, w0, b0, w1, b1 = K.stem_inputs(dtype, npix, "negzero-col")
    assert bool(torch.signbit(w0[:, 5]).all())
    g = Gpu(lib)
    y_neg = g.stem_raw(x8, w0, b0, w1, b1)
    w0p = w0.clone()
    w0p[:, 5] = 0.0
    y_pos = g.stem_raw(x8, w0p, b0, w1, b1)
    assert torch.equal(y_neg.view(torch.int16 if dtype == "float16" else torch.int32), y_pos.view(torch.int16 if dtype == "float16" else torch.int32))


@pytest.mark.parametrize("dtype", K.DTYPES)
def test_tanh_keeps_the_sign_of_zero(lib, dtype):
    x = torch.tensor([0.0, -0.0] * 4, dtype=K.TDT[dtype])
    (y,) = Gpu(lib).tanh(x)
    assert torch.equal(torch.signbit(y), torch.signbit(x)) and bool((y == 0).all())
