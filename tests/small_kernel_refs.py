"""float64 CPU references of the small per-pixel and normalisation kernels (K6 norm.hip, K7 upsample.hip, K8 + image_pad pointwise.hip),
independent of the code under test and of torch's fp32 kernels.

Every function takes numpy float64 arrays holding THE EXACT VALUES THE KERNEL READS: the caller rounds its inputs to the I/O dtype first and
widens them with f64().  Constants that the reference model compares or clamps against on fp32 tensors (0.2, 1e-1, 1e-2, 1e2) are the
np.float32 values, as in the kernels and in torch on fp32 tensors.  Nothing here rounds, except where the operation itself holds an
intermediate in the I/O dtype: the x2 logits of logit_up2 and the stem's hidden layer.
"""
import numpy as np

F32 = np.float32
C_CONF = np.float64(F32(0.2))
C_EPS_G = F32(1e-1)
C_EPS_L = F32(1e-2)
C_100 = np.float64(F32(1e2))


def f64(t):
    """torch tensor / array of any dtype -> numpy float64 (exact for fp16, fp32, uint8)"""
    if hasattr(t, "detach"):
        t = t.detach().cpu()
        t = t.double().numpy() if t.dtype.is_floating_point else t.numpy()
    return np.asarray(t, dtype=np.float64)


def round_to(a, dtype_name):
    """one IEEE round-to-nearest-even to "float16" / "float32", back in float64"""
    return np.asarray(a, dtype=np.float64).astype(dtype_name).astype(np.float64)


def layernorm(x, eps=1e-5):
    """attentions.py:117,148,182,213,243: nn.LayerNorm(dim, elementwise_affine=False) over the last axis -- biased variance, eps 1e-5"""
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + np.float64(F32(eps)))


def groupnorm_nhwc(x, G, gamma, beta, eps=1e-5):
    """submodules.py:80,90: nn.GroupNorm(G, C) with affine; x (N,H,W,C): statistics per (sample, group) over H, W and the group's C/G
    consecutive channels, biased variance"""
    N, H, W, C = x.shape
    xg = x.reshape(N, H * W, G, C // G)
    m = xg.mean((1, 3), keepdims=True)
    v = ((xg - m) ** 2).mean((1, 3), keepdims=True)
    y = ((xg - m) / np.sqrt(v + np.float64(F32(eps)))).reshape(N, H, W, C)
    return y * gamma.reshape(1, 1, 1, C) + beta.reshape(1, 1, 1, C)


def neigh9(m):
    """utils.py:9-20 custom_unfold(kernel 3, padding 1, replicate): m (B,h,w) -> (B,9,h,w), neighbour n = 3 * dy + dx at (y + dy - 1, x + dx - 1)"""
    B, h, w = m.shape
    p = np.pad(m, ((0, 0), (1, 1), (1, 1)), mode="edge")
    return np.stack([p[:, dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], 1)


def _lin_up2(n):
    """ATen upsample_bilinear2d, scale 2, align_corners=False, one axis of length n: src = max((dst + 0.5) / 2 - 0.5, 0) -> (i0, i1, frac)"""
    s = np.maximum((np.arange(2 * n, dtype=np.float64) + 0.5) * 0.5 - 0.5, 0.0)
    i0 = np.floor(s).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, s - i0


def bilinear_up2(x):
    """x (B,h,w,C) -> (B,2h,2w,C): F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) (unet.py:32-37, s2m2.py:126)"""
    y0, y1, ly = _lin_up2(x.shape[1])
    x0, x1, lx = _lin_up2(x.shape[2])
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    top = x[:, y0][:, :, x0] * (1 - lx) + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * (1 - lx) + x[:, y1][:, :, x1] * lx
    return top * (1 - ly) + bot * ly


def convex_upsample(maps, logits, factor, scales=None, logit_up2=False, io_dtype="float32"):
    """s2m2.py:101-133 upsample4x / upsample1x: custom_unfold -> F.interpolate(nearest, factor) -> softmax over the 9 mask logits -> product ->
    sum.  maps: (B,hs,ws) each; logits (B,Ho,Wo,>=9) (channels 0..8 used), or (B,hs,ws,>=9) with logit_up2: the output_upsample branch
    (s2m2.py:123-127) -- bilinear x2 of the logits, whose result the model holds in the activation dtype (rounded to io_dtype here).
    -> list of (B,Ho,Wo); the channel copy of map 0 (chan_out) is outs[0] rounded to the I/O dtype by the caller."""
    lg = logits[..., :9]
    if logit_up2:
        lg = round_to(bilinear_up2(lg), io_dtype)
    e = np.exp(lg - lg.max(-1, keepdims=True))
    wgt = np.moveaxis(e / e.sum(-1, keepdims=True), -1, 1)               # (B,9,Ho,Wo)
    outs = []
    for m, s in zip(maps, scales or [1.0] * len(maps)):
        n9 = neigh9(m)
        n9 = n9.repeat(factor, 2).repeat(factor, 3)                      # nearest: source index = floor(dst / factor)
        outs.append((n9 * wgt).sum(1) * np.float64(F32(s)))
    return outs


def resample2x(x, mode):
    """x (N,H,W,C).  mode 0: nn.AvgPool2d(2) (unet.py:25-30, stacked_MRT.py:22-27); mode 1: nn.Upsample(scale_factor=2, mode='bilinear',
    align_corners=False) (unet.py:32-37, stacked_MRT.py:29-34)"""
    if mode == 0:
        return (x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2]) * 0.25
    return bilinear_up2(x)


def image_prep(img0, img1):
    """s2m2.py:80-89,140-143 normalize_img + left/right concat: (B,3,H,W) in [0,255] x 2 -> (2B,H,W,8); channels 1..3 = (img / 255 - 0.5) * 2,
    the others 0 (the 8-channel NHWC packing of the stem's input)"""
    x = np.concatenate([img0, img1], 0)
    out = np.zeros((x.shape[0], x.shape[2], x.shape[3], 8))
    out[..., 1:4] = np.moveaxis((x / 255.0 - 0.5) * 2.0, 1, -1)
    return out


def logit(p, eps):
    """torch.logit(p, eps) on an fp32 tensor: p clamped to [eps, 1 - eps] with both ends formed in fp32, then log(p / (1 - p))"""
    lo, hi = np.float64(F32(eps)), np.float64(F32(1.0) - F32(eps))
    p = np.clip(p, lo, hi)
    return np.log(p / (1.0 - p))


def refine_prep(disp, conf, occ, mode):
    """refinenet.py:63-68 (mode 0, GlobalRefiner: mask = conf > 0.2; disp / 1e2 * mask; logit(mask * conf, eps=1e-1)) and refinenet.py:134-141
    (mode 1, LocalRefiner: disp / 1e2; logit(conf, eps=1e-2); logit(occ, eps=1e-2)).  (B,h,w) maps -> (B,h,w,8), unused channels 0"""
    out = np.zeros(disp.shape + (8,))
    if mode == 0:
        mask = (conf > C_CONF).astype(np.float64)
        out[..., 0] = disp / C_100 * mask
        out[..., 1] = logit(mask * conf, C_EPS_G)
    else:
        out[..., 0] = disp / C_100
        out[..., 1] = logit(conf, C_EPS_L)
        out[..., 2] = logit(occ, C_EPS_L)
    return out


def global_update(upd0, disp, conf, clamp0):
    """refinenet.py:70-71, s2m2.py:160-161: disp = mask * disp + (1 - mask) * update * 1e2 [, clamp(min=0)], mask = conf > 0.2; upd0 = channel 0"""
    mask = (conf > C_CONF).astype(np.float64)
    d = mask * disp + (1.0 - mask) * (upd0 * C_100)
    return np.maximum(d, 0.0) if clamp0 else d


def refine_update(dco, disp, conf, occ, use_positivity):
    """refinenet.py:149-151, s2m2.py:177-180: disp += dco[0]; conf = sigmoid(dco[8] + logit(conf, 1e-2)); occ = sigmoid(dco[9] + logit(occ,
    1e-2)); disp.clamp(min=0) with use_positivity; occ *= (x - disp >= 0), x the pixel's column.  dco (B,h,w,>=10) -> (disp, conf, occ).
    small_next, the side input of the next iteration, is refine_prep(mode 1) of the three fp32 maps THE KERNEL WROTE (the exact values it
    reads back next iteration): the caller evaluates refine_prep on those, not on these float64 maps -- logit amplifies a last-bit
    difference of conf near 0.99 a hundredfold, which is the update's error, not the side input's"""
    d = disp + dco[..., 0]
    c = 1.0 / (1.0 + np.exp(-(dco[..., 8] + logit(conf, C_EPS_L))))
    o = 1.0 / (1.0 + np.exp(-(dco[..., 9] + logit(occ, C_EPS_L))))
    if use_positivity:
        d = np.maximum(d, 0.0)
    x = np.arange(disp.shape[-1], dtype=np.float64).reshape((1,) * (disp.ndim - 1) + (-1,))
    o = o * (x - d >= 0)
    return d, c, o


def tanh(x):
    """s2m2.py:166: hidden = torch.tanh(ctx0)"""
    return np.tanh(x)


def _erf(x):
    import math
    return np.vectorize(math.erf, otypes=[np.float64])(x)


def stem_mlp(x8, w0, b0, w1, b1, io_dtype):
    """submodules.py:68-71: conv0 = Conv2d(3,16,1) - GELU (erf) - Conv2d(16,16,1) per pixel on the 8-channel packed input; the 16-channel
    intermediate is rounded to the I/O dtype after the GELU (where the separate layers store it).  x8 (npix,8), w0 (16,8), w1 (16,16)"""
    h = x8 @ w0.T + b0
    h = round_to(0.5 * h * (1.0 + _erf(h / np.sqrt(2.0))), io_dtype)
    return h @ w1.T + b1


def image_pad(img, factor=32):
    """image_utils.py:27-71 image_pad: zero-pad (B,C,H,W) to multiples of factor (left / top get floor(pad / 2)), adaptive_avg_pool2d of the
    padded image to (H // factor, W // factor), F.interpolate(size=(Hn, Wn), mode='bilinear') of that, the original pasted back in the middle"""
    B, C, H, W = img.shape
    Hn, Wn = -(-H // factor) * factor, -(-W // factor) * factor
    ph, pw = Hn - H, Wn - W
    x = np.zeros((B, C, Hn, Wn))
    x[:, :, ph // 2: ph // 2 + H, pw // 2: pw // 2 + W] = img
    Ho, Wo = H // factor, W // factor
    down = np.zeros((B, C, Ho, Wo))
    for i in range(Ho):
        y0, y1 = (i * Hn) // Ho, -(-((i + 1) * Hn) // Ho)
        for j in range(Wo):
            x0, x1 = (j * Wn) // Wo, -(-((j + 1) * Wn) // Wo)
            down[:, :, i, j] = x[:, :, y0:y1, x0:x1].mean((2, 3))

    def axis(n_in, n_out):                                              # align_corners=False, scale = n_in / n_out
        s = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5, 0.0)
        i0 = np.floor(s).astype(np.int64)
        return i0, np.minimum(i0 + 1, n_in - 1), s - i0
    y0, y1, ly = axis(Ho, Hn)
    x0, x1, lx = axis(Wo, Wn)
    ly, lx = ly[None, None, :, None], lx[None, None, None, :]
    top = down[:, :, y0][:, :, :, x0] * (1 - lx) + down[:, :, y0][:, :, :, x1] * lx
    bot = down[:, :, y1][:, :, :, x0] * (1 - lx) + down[:, :, y1][:, :, :, x1] * lx
    out = top * (1 - ly) + bot * ly
    out[:, :, ph // 2: ph // 2 + H, pw // 2: pw // 2 + W] = img
    return out
