"""Cases, inputs, the float64 reference, the elementwise bound and the one comparator of the K5 (s2m2_conv2d, csrc/conv.hip) strided and
many-tap tests, shared by tests/test_hip_k5_strided.py (the kernel, on every tile id of the igemm / igemm2 families) and
tests/test_k5_cases_cpu.py (the construction without the kernel: what agrees with torch's own fp32 conv, holds its representability claim
and rejects eight wrong loaders on the CPU is literally what the GPU test asserts).

What is under test is the loader of the v1 kernel (ConvLoader) and of its v2 twin: output row m -> (n, yo, xo), window centre
(yo * stride, xo * stride), Ho = ceil(H / stride), a mask of up to 32 taps per row, a flat pixel index plus a tap offset, the K cursor
(K order 0 and 1) and the choice of source and pixel stride per K piece.  A wrong mask bit does not fault: it reads the neighbouring row
or image.  So the inputs are made to show it.

Layers (LAYERS)  3x3 s2 128 -> 128 and 192 -> 192, 5x5 s2 16 -> 64 (K = 400 ends inside a K tile) and 128 -> 128, 5x5 s1, 1x1 s2 (pure
                 subsampling), 3x1 / 1x3 s2, 1x7 / 7x3 s1, 1x31 s1 on W = 5 (tap bit 30, most taps outside), 3x3 s2 on sources [8, 128] that
                 are channel slices of tensors of different width, 3x3 s2 128 -> 136 (Cout tail), 3x3 s2 32 -> 128 on the two grids next to
                 the heuristic's t20_min threshold (304 and 296 tiles of 128 x 128).
Shapes           (1,1,1) (1,2,2) (1,1,9) (1,9,1) (1,2,5): windows mostly outside; (1,9,13) (1,8,12) (1,9,12): odd / even mixes below one
                 tile; (3,11,15): M = 144, tiles straddle output rows and images; (2,16,16): M = 128, no tail; (1,33,61): M = 527, several
                 tiles and a ragged last group.  Every shape meets 3x3 s2 and 5x5 s2.
Operands         rounded once to the I/O dtype on the CPU; kernel and reference read the rounded values.  Bias is fp32.  On the device every
                 source is the channel slice [PAD, PAD + c) of images 1 .. N of an (N + 2, H, W, c + 2 PAD) buffer whose every other element
                 is NaN (wide()): a read that should have been zero padding, or that runs past Cin, makes the output NaN.
Reference        F.conv2d in float64, stride, padding (KH // 2, KW // 2), on the channel concatenation; activation, out_scale and epilogue in
                 float64.  Its size is asserted to be ceil(H / s) x ceil(W / s).

`exact` regime   integer activations (+-1, +-2; +-1 where 2 K + 8 > 2048), weights in {-1, 0, 1} thinned to at most 2040 / max |x| non-zeros per
                 output channel, integer bias |b| <= 8, activation NONE or RELU, out_scale 1.  Then sum |w| |x| + |b| <= 2048 per element in
                 the worst case: every partial sum in any order and the result are integers of at most 2048, exact in fp16 and in fp32; fp16
                 products are exact in fp32.  build() asserts S <= 2048 and reference() asserts ref.to(dtype) == ref.  The kernel must equal
                 the reference bit for bit (+0.0 for zero: an fp32 chain that starts at +0 never yields -0).  One wrong, missing or extra tap
                 changes an integer.
`gauss` regime   activations N(0.3, 1), weights N(0, 1 / K), bias N(0, 0.1^2); NONE, RELU, GELU; out_scale 1 or 0.5; epilogues ADD, MUL, GRU,
                 GATEMIX with operands indexed by the OUTPUT pixel.  Bound per element (bound()), nothing measured -- u = 2^-24, K = KH KW Cin,
                 S = conv(|x|, |w|) + |b|:
                   accumulation      (K + 2) u S: an fp32 chain of K terms in any order, one product rounding (fp32 mode) and the bias add
                   activation        times its Lipschitz constant (1, 1, 1.13 for GELU) plus its own error: 0, 0, and for GELU the absolute
                                     figures of csrc/epilogue.h -- 3.3e-7 (fast_gelu, fp32) / 8.1e-7 (fast_gelu16) -- and for the fp16 GELU
                                     one fp16 ulp of the result (tests/test_gelu16_cpu.py: within one ulp of the correctly rounded value);
                                     the figures hold on [-8, 8], and build() asserts the pre-activations stay inside;
                                     SIGMOID and TANH (the patch-kernel cases of tests/k5_patch_cases.py): Lipschitz constants 1 / 4 and 1,
                                     own error act_abs(), derived in its docstring from epilogue.h's two formulas (about 4 u and 9 u at most)
                   out_scale         times out_scale
                   staging           half an ulp of the I/O dtype at the value: the kernel stages act(.) * scale in the I/O dtype
                   epilogue          v the staged value with error e, a0 / a1 the operands, the arithmetic in fp32 (3 u per term at most):
                                     ADD e + u |o|;  MUL |a0| e + u |o|;  GRU |a0| e + 3 u (|1 - a0| |a1| + |a0| |v|);
                                     GATEMIX (|a0| + |a1|) e + 3 u (|g a0| + |(1 - g) a1|), the clamp has Lipschitz constant 1;
                                     then half an ulp of the I/O dtype at the result again.
                 Half an ulp is taken at |value| + error so far, the largest magnitude the kernel can be rounding.  If a correct kernel
                 exceeds the bound, a rounding is missing above: find it and write it down.
Comparator       compare(): every element is judged, non-finite fails; the result carries the worst err / bound and its (image, output row,
                 output column, cout).
Wrong loaders    wrong(): the same layer computed with one defect of the kind this loader can have (VARIANTS): Ho = floor(H / 2); the window
                 centred on 2 y + 1; padding K // 2 - 1; a tap left or right of the image reads the flat index (the neighbouring row's
                 pixel); a tap above or below reads the neighbouring image; tap bits 16 and up treated as outside; K order 1 weights read as
                 K order 0; the second source's pixel stride taken from the first.  differs() says on which cases a variant differs by
                 construction.
"""
import collections
import functools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from s2m2_amd import pack

TDT = {"float32": torch.float32, "float16": torch.float16}
SHORT = {"float32": "fp32", "float16": "fp16"}
U24 = 2.0 ** -24
ACT_NONE, ACT_GELU, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3, 4     # s2m2_amd.hip.ACT_*
EPI_NONE, EPI_ADD, EPI_MUL, EPI_GRU, EPI_GATEMIX = 0, 1, 2, 3, 4        # s2m2_amd.hip.EPI_*
ACT_NAME = {ACT_NONE: "none", ACT_GELU: "gelu", ACT_RELU: "relu", ACT_SIGMOID: "sigmoid", ACT_TANH: "tanh"}
EPI_NAME = {EPI_NONE: "", EPI_ADD: "add", EPI_MUL: "mul", EPI_GRU: "gru", EPI_GATEMIX: "gatemix"}
LIPSCHITZ = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_GELU: 1.13, ACT_SIGMOID: 0.25, ACT_TANH: 1.0}
GELU_ABS = {"float32": 3.3e-7, "float16": 8.1e-7}                       # csrc/epilogue.h
GELU_RANGE = 8.0
EXP_RANGE = 8.0                                                         # |pre-activation| of a SIGMOID / TANH case: act_abs() is derived for it
EXACT_MAX = 2048                                                        # integers up to here are fp16 values
PAD = 8                                                                 # channels of NaN on either side of a source inside its buffer
TILES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 20, 21, 22, 27)   # 0 and every id conv_select.h maps to igemm / igemm2

Layer = collections.namedtuple("Layer", "KH KW stride cs Cout")
LAYERS = {
    "3x3s2_128": Layer(3, 3, 2, (128,), 128),            # cnn_backbone.conv2_down.0
    "3x3s2_192": Layer(3, 3, 2, (192,), 192),
    "5x5s2_16_64": Layer(5, 5, 2, (16,), 64),            # cnn_backbone.conv1_down.0: K = 400
    "5x5s1_16_64": Layer(5, 5, 1, (16,), 64),
    "5x5s2_128": Layer(5, 5, 2, (128,), 128),
    "1x1s2_32_64": Layer(1, 1, 2, (32,), 64),
    "3x1s2_32_64": Layer(3, 1, 2, (32,), 64),
    "1x3s2_32_64": Layer(1, 3, 2, (32,), 64),
    "1x7s1_32_64": Layer(1, 7, 1, (32,), 64),
    "7x3s1_32_64": Layer(7, 3, 1, (32,), 64),
    "1x31s1_32_64": Layer(1, 31, 1, (32,), 64),
    "3x3s2_8+128": Layer(3, 3, 2, (8, 128), 128),
    "3x3s2_128_136": Layer(3, 3, 2, (128,), 136),
    "3x3s2_32_128": Layer(3, 3, 2, (32,), 128),
}
SHAPES = ((1, 1, 1), (1, 2, 2), (1, 1, 9), (1, 9, 1), (1, 2, 5), (1, 9, 13), (1, 8, 12), (1, 9, 12), (3, 11, 15), (2, 16, 16), (1, 33, 61))
T20_ABOVE, T20_BELOW = (2, 256, 304), (2, 256, 296)                    # 3x3s2_32_128: 304 and 296 tiles of 128 x 128 (t20_min = 300)

Spec = collections.namedtuple("Spec", "layer shape regime act scale epi tiles epi_cout0", defaults=(0,))


def _specs():
    s = {}

    def add(layer, shape, regime, act=ACT_NONE, scale=1.0, epi=EPI_NONE, tiles=TILES):
        name = f"{layer}-{'x'.join(map(str, shape))}-{regime}"
        if regime == "gauss":
            name += f"-{ACT_NAME[act]}" + (f"-x{scale:g}" if scale != 1.0 else "") + (f"-{EPI_NAME[epi]}" if epi else "")
        elif act:
            name += f"-{ACT_NAME[act]}"
        assert name not in s, name
        s[name] = Spec(layer, shape, regime, act, scale, epi, tiles)

    for i, shape in enumerate(SHAPES):                                  # every shape on the two layers the forward runs strided
        add("3x3s2_128", shape, "exact", ACT_RELU if i % 2 else ACT_NONE)
        add("5x5s2_16_64", shape, "exact", ACT_NONE if i % 2 else ACT_RELU)
    for shape, act, scale in (((1, 9, 13), ACT_RELU, 1.0), ((3, 11, 15), ACT_NONE, 0.5), ((2, 16, 16), ACT_GELU, 1.0), ((1, 33, 61), ACT_RELU, 0.5)):
        add("3x3s2_128", shape, "gauss", act, scale)
    for shape, scale in (((1, 2, 5), 1.0), ((3, 11, 15), 0.5), ((1, 33, 61), 1.0)):
        add("5x5s2_16_64", shape, "gauss", ACT_GELU, scale)
    add("5x5s2_128", (1, 9, 13), "exact")
    add("5x5s2_128", (3, 11, 15), "exact", ACT_RELU)
    add("5x5s2_128", (1, 33, 61), "gauss", ACT_NONE)
    add("3x3s2_192", (3, 11, 15), "exact")
    add("3x3s2_192", (1, 9, 12), "gauss", ACT_RELU)
    add("5x5s1_16_64", (3, 11, 15), "exact")
    add("5x5s1_16_64", (1, 9, 13), "gauss", ACT_GELU)
    add("1x1s2_32_64", (3, 11, 15), "exact")
    add("1x1s2_32_64", (1, 1, 9), "exact", ACT_RELU)
    add("1x1s2_32_64", (1, 9, 12), "gauss", ACT_NONE, 0.5)
    add("3x1s2_32_64", (3, 11, 15), "exact")
    add("3x1s2_32_64", (1, 9, 1), "exact")
    add("1x3s2_32_64", (3, 11, 15), "exact")
    add("1x3s2_32_64", (1, 1, 9), "exact")
    add("1x7s1_32_64", (3, 11, 15), "exact")
    add("1x7s1_32_64", (1, 2, 5), "exact")
    add("1x7s1_32_64", (1, 9, 13), "gauss", ACT_RELU)
    add("7x3s1_32_64", (3, 11, 15), "exact")
    add("7x3s1_32_64", (1, 2, 5), "exact")
    add("7x3s1_32_64", (1, 9, 13), "gauss", ACT_GELU)
    add("1x31s1_32_64", (1, 2, 5), "exact")
    add("1x31s1_32_64", (3, 4, 5), "exact", ACT_RELU)
    add("1x31s1_32_64", (1, 2, 5), "gauss", ACT_NONE)
    add("3x3s2_8+128", (3, 11, 15), "exact")
    add("3x3s2_8+128", (1, 33, 61), "exact", ACT_RELU)
    add("3x3s2_8+128", (1, 9, 13), "gauss", ACT_GELU)
    add("3x3s2_128_136", (3, 11, 15), "exact")
    add("3x3s2_128_136", (1, 9, 12), "gauss", ACT_RELU)
    add("3x3s2_128", (3, 11, 15), "gauss", ACT_NONE, 1.0, EPI_ADD)
    add("3x3s2_128", (3, 11, 15), "gauss", ACT_RELU, 1.0, EPI_MUL)
    add("3x3s2_128", (3, 11, 15), "gauss", ACT_NONE, 0.5, EPI_GRU)
    add("3x3s2_128", (3, 11, 15), "gauss", ACT_NONE, 1.0, EPI_GATEMIX)
    add("3x3s2_32_128", T20_ABOVE, "exact", tiles=(0,))                 # the heuristic's own picks: tile 20 above t20_min, tile 6 below
    add("3x3s2_32_128", T20_BELOW, "exact", tiles=(0,))
    return s


SPECS = _specs()
NAMES = tuple(SPECS)
SMALL = tuple(n for n in NAMES if len(SPECS[n].tiles) > 1)             # all but the two heuristic grids

Case = collections.namedtuple("Case", "name spec layer dtype N H W Ho Wo Cin K xs w b a0 a1")   # CPU float32 tensors holding I/O dtype values


def out_size(H, W, stride):
    return -(-H // stride), -(-W // stride)


def korder1_ok(case):
    """K order 1 needs Cin to be whole chunks of 64 bytes of channels"""
    return case.Cin % pack.chunk_channels(TDT[case.dtype]) == 0


@functools.lru_cache(maxsize=None)
def build(name, dtype="float16"):
    """built once per process and shared; nothing may write into it"""
    return build_case(name, SPECS[name], LAYERS[SPECS[name].layer], dtype)


def build_case(name, spec, L, dtype):
    """the operands of one (spec, layer), seeded by the name (tests/k5_patch_cases.py builds its own specs with it)"""
    N, H, W = spec.shape
    Ho, Wo = out_size(H, W, L.stride)
    Cin, K = sum(L.cs), L.KH * L.KW * sum(L.cs)
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    rnd = lambda t: t.to(TDT[dtype]).float()
    a0 = a1 = None
    if spec.regime == "exact":
        assert spec.act in (ACT_NONE, ACT_RELU) and spec.scale == 1.0 and spec.epi == EPI_NONE
        xmax = 2 if 2 * K + 8 <= EXACT_MAX else 1
        nnz = min(K, (EXACT_MAX - 8) // xmax)
        xs = [(torch.randint(1, xmax + 1, (N, H, W, c), generator=g) * (2 * torch.randint(0, 2, (N, H, W, c), generator=g) - 1)).float() for c in L.cs]
        w = torch.randint(-1, 2, (L.Cout, K), generator=g).float()
        if nnz < K:                                                     # thinned: the nnz columns of lowest random rank stay
            w = w * (torch.rand(L.Cout, K, generator=g).argsort(1).argsort(1) < nnz)
        w = w.reshape(L.Cout, L.KH, L.KW, Cin).permute(0, 3, 1, 2).contiguous()
        b = torch.randint(-8, 9, (L.Cout,), generator=g).float()
    else:
        xs = [rnd(torch.randn(N, H, W, c, generator=g) + 0.3) for c in L.cs]
        w = rnd(torch.randn(L.Cout, Cin, L.KH, L.KW, generator=g) / math.sqrt(K))
        b = torch.randn(L.Cout, generator=g) * 0.1
        assert spec.epi_cout0 == 0 or (spec.epi in (EPI_ADD, EPI_MUL) and 0 < spec.epi_cout0 < L.Cout)
        if spec.epi in (EPI_ADD, EPI_GATEMIX):
            a0 = rnd(torch.randn(N, Ho, Wo, L.Cout - spec.epi_cout0, generator=g))
        elif spec.epi in (EPI_MUL, EPI_GRU):
            a0 = rnd(torch.rand(N, Ho, Wo, L.Cout - spec.epi_cout0, generator=g))   # a gate
        if spec.epi in (EPI_GRU, EPI_GATEMIX):
            a1 = rnd(torch.randn(N, Ho, Wo, L.Cout, generator=g))
    for t in xs + [w]:
        assert torch.equal(t, rnd(t))
    c = Case(name, spec, L, dtype, N, H, W, Ho, Wo, Cin, K, tuple(xs), w, b, a0, a1)
    if spec.regime == "exact":
        S = _conv64([x.abs() for x in xs], w.abs(), L) + b.abs().double()
        assert float(S.max()) <= EXACT_MAX, (name, float(S.max()))
    elif spec.act in (ACT_SIGMOID, ACT_TANH):                           # the range act_abs() is derived for
        top = float((_conv64(xs, w, L) + b.double()).abs().max())
        assert top <= EXP_RANGE, (name, top)
    return c


def widen(x, poison=float("nan")):
    """an (N, H, W, c) tensor as the GPU tests lay it out: (N + 2, H, W, c + 2 PAD) with the values at [1 : 1 + N, :, :, PAD : PAD + c], `poison` elsewhere"""
    N, H, W, c = x.shape
    big = torch.full((N + 2, H, W, c + 2 * PAD), poison)
    big[1:1 + N, :, :, PAD:PAD + c] = x
    return big


def in_nan(t):
    """a device tensor t (N, H, W, c) as images 1 .. N of an (N + 2)-image buffer and the middle third of a tensor three times as wide, NaN
    everywhere else -> (buffer, view); the fused kernels' tests (K14, K17, K19) lay their inputs out like this"""
    N, H, W, c = t.shape
    big = torch.full((N + 2, H, W, 3 * c), float("nan"), device=t.device, dtype=t.dtype)
    view = big[1:1 + N, :, :, c:2 * c]
    view.copy_(t)
    assert view.stride(2) == 3 * c and not view.is_contiguous() and bool(torch.isnan(big[0]).all()) and bool(torch.isnan(big[-1]).all())
    return big, view


def wide(case, i, poison=float("nan")):
    """source i as the GPU test lays it out: (N + 2, H, W, c + 2 PAD) with the values at [1 : 1 + N, :, :, PAD : PAD + c] and `poison` elsewhere"""
    return widen(case.xs[i], poison)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def _conv64(xs, w, L):
    x = torch.cat([t.double() for t in xs], -1).permute(0, 3, 1, 2)
    y = F.conv2d(x, w.double(), None, stride=L.stride, padding=(L.KH // 2, L.KW // 2)).permute(0, 2, 3, 1)
    Ho, Wo = out_size(x.shape[2], x.shape[3], L.stride)
    assert tuple(y.shape[1:3]) == (Ho, Wo), (tuple(y.shape), Ho, Wo)
    return y


def activate(pre, act):
    if act == ACT_SIGMOID:
        return torch.sigmoid(pre)
    if act == ACT_TANH:
        return torch.tanh(pre)
    return F.gelu(pre) if act == ACT_GELU else pre.clamp(min=0) if act == ACT_RELU else pre


def act_abs(x, act):
    """The absolute error of the device's own SIGMOID / TANH at the fp32 pre-activation x (float64 tensor), before any rounding to the I/O
    dtype, derived from the two formulas of csrc/epilogue.h; first order in u = 2^-24, |x| <= EXP_RANGE (build_case() asserts it).

    What rounds.  A correctly rounded fp32 operation has relative error u.  v_exp_f32 and v_rcp_f32 are within one ulp of the true value
    (epilogue.h), so each returns the correctly rounded value or one of its two neighbours: at most 1.5 ulp = 3 u relative from the true
    value (an ulp is at most 2 u relative).  L = fl(log2 e) is within u of log2 e.

    SIGMOID  rcp(1 + exp2(fl(-x L))).  fl(-x L) = -x log2 e (1 + d), |d| <= 2 u (the constant and the product), an absolute error of
             2 u |x| log2 e in the exponent, which exp2 turns into a relative error 2 u |x| ln 2 log2 e = 2 u |x| of E = e^-x; with exp2's own
             3 u:  E (1 + (3 + 2 |x|) u).  s = sigmoid(x) = 1 / (1 + E) moves by E / (1 + E)^2 = s (1 - s) per unit of relative error of E:
             s (1 - s) (3 + 2 |x|) u.  The add 1 + E rounds (u) and rcp adds 3 u, both relative to s:  4 u s.
               error <= u [ s (1 - s) (3 + 2 |x|) + 4 s ]                        (at most 4.2 u on [-8, 8]; below (4 + |x|) u everywhere)
    TANH     1 - 2 rcp(1 + exp2(fl(2 x L))), 2 x exact.  E = e^2x (1 + (3 + 4 |x|) u) by the same steps.  q = 2 / (1 + E) = 1 - t, t = tanh(x),
             moves by 2 E / (1 + E)^2 = (1 - t^2) / 2 per unit of relative error of E; the add and rcp give 4 u q; 2 rcp is exact and the last
             subtraction rounds the result (u |t|).
               error <= u [ (1 - t^2) / 2 (3 + 4 |x|) + 4 (1 - t) + |t| ]        (9 u at x = -8, 5.5 u at 0, u at +8; below (8 + 4 |x|) u)
    The second-order terms are below (20 u)^2 < 2e-5 u on the range; 0.01 u is added for them.  tests/test_k5_patch_cases_cpu.py holds both
    figures against a float32 restatement in which exp2 and the reciprocal are each moved by -1, 0 and +1 ulp."""
    ax = x.abs()
    if act == ACT_SIGMOID:
        s = torch.sigmoid(x)
        return U24 * (s * (1 - s) * (3 + 2 * ax) + 4 * s + 0.01)
    if act == ACT_TANH:
        t = torch.tanh(x)
        return U24 * ((1 - t * t) / 2 * (3 + 4 * ax) + 4 * (1 - t) + t.abs() + 0.01)
    raise KeyError(act)


GATE_LO, GATE_HI = float(np.float32(0.01)), float(np.float32(0.99))      # the kernel's clamp constants are fp32


def finish(case, pre):
    """pre-activation (with bias) float64 -> the layer's output: activation, out_scale, epilogue.  spec.epi_cout0 > 0 (two stacked layers in
    one launch): output channels below it get bias and activation only, those from it on the epilogue, whose operand has Cout - epi_cout0 channels"""
    c0 = case.spec.epi_cout0
    if c0:
        return torch.cat([_finish(case, pre[..., :c0], EPI_NONE), _finish(case, pre[..., c0:], case.spec.epi)], -1)
    return _finish(case, pre, case.spec.epi)


def _finish(case, pre, e):
    v = activate(pre, case.spec.act) * case.spec.scale
    if e == EPI_NONE:
        return v
    a0 = case.a0.double()
    if e == EPI_ADD:
        return v + a0
    if e == EPI_MUL:
        return v * a0
    a1 = case.a1.double()
    if e == EPI_GRU:
        return (1 - a0) * a1 + a0 * v
    gt = v.clamp(GATE_LO, GATE_HI)
    return gt * a0 + (1 - gt) * a1


def ulp(v, dtype):
    """the spacing of `dtype` at magnitude |v| (float64 tensor)"""
    if dtype == "float16":
        e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -14)))
        return torch.exp2(e - 10)
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -126)))
    return torch.exp2(e - 23)


def bound(case, pre, S):
    """the elementwise bound of the docstring; pre, S float64 (N, Ho, Wo, Cout).  SIGMOID and TANH: Lipschitz constants 1 / 4 and 1, their own
    error act_abs() (derived there).  spec.epi_cout0: the channels below it are bounded as a layer without epilogue."""
    c0 = case.spec.epi_cout0
    if c0:
        return torch.cat([_bound(case, pre[..., :c0], S[..., :c0], EPI_NONE), _bound(case, pre[..., c0:], S[..., c0:], case.spec.epi)], -1)
    return _bound(case, pre, S, case.spec.epi)


def _bound(case, pre, S, epi):
    spec, dt = case.spec, case.dtype
    half = lambda value, err: 0.5 * ulp(value.abs() + err, dt)
    act = activate(pre, spec.act)
    e = (case.K + 2) * U24 * S * LIPSCHITZ[spec.act]
    if spec.act == ACT_GELU:
        e = e + GELU_ABS[dt]
        if dt == "float16":
            e = e + ulp(act.abs() + e, dt)
    elif spec.act in (ACT_SIGMOID, ACT_TANH):
        e = e + act_abs(pre, spec.act)
    e = e * spec.scale
    v = act * spec.scale
    e = e + half(v, e)
    if epi == EPI_NONE:
        return e
    o = _finish(case, pre, epi)
    a0 = case.a0.double().abs()
    if epi == EPI_ADD:
        e = e + U24 * (o.abs() + e)
    elif epi == EPI_MUL:
        e = a0 * e + U24 * (o.abs() + a0 * e)
    else:
        a1 = case.a1.double().abs()
        if epi == EPI_GRU:
            terms = (1 - case.a0.double()).abs() * a1 + a0 * (v.abs() + e)
            e = a0 * e + 3 * U24 * terms
        else:
            gt = v.clamp(GATE_LO, GATE_HI)
            e = (a0 + a1) * e + 3 * U24 * ((gt + e) * a0 + (1 - gt + e) * a1)
    return e + half(o, e)


Ref = collections.namedtuple("Ref", "out bound pre")                    # bound None: the exact regime


@functools.lru_cache(maxsize=None)
def reference(name, dtype="float16"):
    """computed once per process and shared"""
    return reference_case(build(name, dtype))


def reference_case(c):
    name, dtype = c.name, c.dtype
    pre = _conv64(c.xs, c.w, c.layer) + c.b.double()
    out = finish(c, pre) + 0.0                                          # (-0.0 -> +0.0)
    assert out.dtype == torch.float64 and tuple(out.shape) == (c.N, c.Ho, c.Wo, c.layer.Cout)
    if c.spec.regime == "exact":
        assert torch.equal(out.to(TDT[dtype]).double(), out), name       # representable: the kernel owes every bit
        return Ref(out, None, pre)
    if c.spec.act == ACT_GELU:
        assert float(pre.abs().max()) <= GELU_RANGE, (name, float(pre.abs().max()))
    S = _conv64([x.abs() for x in c.xs], c.w.abs(), c.layer) + c.b.abs().double()
    return Ref(out, bound(c, pre, S), pre)


# ---- the comparator -----------------------------------------------------------------------------------------------------------------------
Result = collections.namedtuple("Result", "ratio where bad")            # ratio: worst err / bound (exact regime: 0.0 or inf)


def compare(case, ref, got):
    """one output (N, Ho, Wo, Cout) of any float dtype against a Ref: every element within its bound (exact regime: the same value, and no -0.0).
    bad: what fails (empty: the run passes)."""
    want = ref.out
    g = got.detach().cpu()
    if tuple(g.shape) != tuple(want.shape):
        return Result(float("inf"), None, [f"shape {tuple(g.shape)}, expected {tuple(want.shape)}"])
    gd = g.double()
    if ref.bound is None:
        miss = ~(gd == want) | ((gd == 0) & torch.signbit(gd))
        ratio = torch.where(miss, float("inf"), 0.0).double()
    else:
        ratio = (gd - want).abs() / ref.bound
        ratio = torch.where(torch.isfinite(gd), ratio, torch.full_like(ratio, float("inf")))
    at = int(ratio.argmax())
    where = tuple(int(i) for i in np.unravel_index(at, tuple(want.shape)))
    worst = float(ratio.reshape(-1)[at])
    bad = []
    if not worst <= 1.0:
        n = int((~(ratio <= 1.0)).sum())
        kind = "differ from the reference" if ref.bound is None else "over the bound"
        bad.append(f"{n} elements {kind}, worst err / bound {worst:.3g} at (image, row, column, cout) = {where}: "
                   f"got {float(gd[where])!r}, expected {float(want[where])!r}")
    return Result(worst, where, bad)


def verdict(case, res):
    if case.spec.regime == "exact":
        return "bit-equal" if res.ratio == 0.0 else f"DIFFERS at {res.where}"
    return f"err / bound {res.ratio:5.3f}" + (f" at {res.where}" if res.ratio > 1.0 else "")


def line(case, what, *results):
    """one line of the table: a run (or the K order 0 and K order 1 runs of one tile) of a case"""
    return f"{case.name:44s} {SHORT[case.dtype]}  {what:16s} " + "   ".join(verdict(case, r) if r is not None else "-" for r in results)


# ---- wrong loaders ------------------------------------------------------------------------------------------------------------------------
VARIANTS = ("floor_ho", "centre_2y1", "pad_less", "row_wrap", "image_wrap", "taps_16", "korder1_as_0", "stride_of_src0")


def differs(case, variant):
    """the variant computes something else than the layer on this case, by construction"""
    L = case.layer
    if variant == "floor_ho":
        return L.stride == 2 and (case.H % 2 == 1 or case.W % 2 == 1)
    if variant == "centre_2y1":
        return L.stride == 2
    if variant == "pad_less":
        return L.KH >= 3 or L.KW >= 3
    if variant == "row_wrap":                                            # a row above or below to wrap into; stride 2 on an even W has no tap at x = W
        return L.KW >= 3 and case.N * case.H > 1
    if variant == "image_wrap":
        return L.KH >= 3 and case.N > 1
    if variant == "taps_16":                                             # a tap of index 16 or more that is inside the image for some output pixel
        ys, xs = range(0, case.H, L.stride), range(0, case.W, L.stride)
        return any(a * L.KW + b >= 16 and any(0 <= y + a - L.KH // 2 < case.H for y in ys) and any(0 <= x + b - L.KW // 2 < case.W for x in xs)
                   for a in range(L.KH) for b in range(L.KW))
    if variant == "korder1_as_0":
        return korder1_ok(case) and L.KW >= 3 and case.Cin > pack.chunk_channels(TDT[case.dtype])
    if variant == "stride_of_src0":
        return len(L.cs) > 1
    raise KeyError(variant)


def korder1_weights_read_as_0(case):
    """the layer's weights packed in K order 1, unpacked as if they were K order 0 -> (Cout, Cin, KH, KW)"""
    L = case.layer
    wp = pack.pack_conv(case.w, torch.float32, [(c, c) for c in L.cs], korder=0)
    ch = pack.chunk_channels(TDT[case.dtype])
    w1 = wp.reshape(L.Cout, L.KH, L.KW, case.Cin // ch, ch).permute(0, 1, 3, 2, 4).reshape(L.Cout, L.KH, L.KW, case.Cin)
    return w1.permute(0, 3, 1, 2).contiguous()


def wrong(case, variant=None):
    """the layer by an explicit gather per tap, as the loader addresses it: flat pixel index of the window centre plus a tap offset, a mask per
    tap.  variant None is the layer itself (tests/test_k5_cases_cpu.py compares it with the reference); the others are VARIANTS."""
    L = case.layer
    N, H, W, s = case.N, case.H, case.W, L.stride
    x = torch.cat([t.double() for t in case.xs], -1)
    w = (korder1_weights_read_as_0(case) if variant == "korder1_as_0" and korder1_ok(case) else case.w).double()
    if variant == "stride_of_src0":                                      # source i >= 1 addressed with source 0's pixel stride inside its own buffer
        cols, st0 = [case.xs[0].double()], case.xs[0].shape[-1] + 2 * PAD
        for i in range(1, len(L.cs)):
            big = wide(case, i, poison=3.0).double()
            base = big[1:].reshape(-1)[PAD:]                             # from the source's first element on
            pix = torch.arange(N * H * W)[:, None] * st0 + torch.arange(L.cs[i])[None, :]
            cols.append(base[pix].reshape(N, H, W, L.cs[i]))
        x = torch.cat(cols, -1)
    Ho, Wo = out_size(H, W, s)
    if variant == "floor_ho" and s == 2:
        Ho, Wo = H // 2, W // 2
    shift = 1 if (variant == "centre_2y1" and s == 2) else 0
    ph, pw = L.KH // 2, L.KW // 2
    if variant == "pad_less":
        ph, pw = max(ph - 1, 0), max(pw - 1, 0)
    P = N * H * W
    flat = torch.cat([x.reshape(P, case.Cin), torch.zeros(1, case.Cin, dtype=torch.float64)])
    n = torch.arange(N)[:, None, None]
    yo = (torch.arange(Ho) * s + shift)[None, :, None]
    xo = (torch.arange(Wo) * s + shift)[None, None, :]
    acc = torch.zeros(N, Ho, Wo, L.Cout, dtype=torch.float64)
    for a in range(L.KH):
        for b in range(L.KW):
            if variant == "taps_16" and a * L.KW + b >= 16:
                continue
            yy, xx = yo + a - ph, xo + b - pw
            iny, inx = (yy >= 0) & (yy < H), (xx >= 0) & (xx < W)
            idx = (n * H + yy) * W + xx
            inbuf = (idx >= 0) & (idx < P)
            ok = iny & inx
            if variant == "row_wrap":
                ok = iny & inbuf
            elif variant == "image_wrap":
                ok = inx & inbuf
            acc += flat[torch.where(ok, idx, torch.full_like(idx, P))] @ w[:, :, a, b].T
    pre = acc + case.b.double()
    if tuple(pre.shape[1:3]) != (case.Ho, case.Wo):
        return activate(pre, case.spec.act) * case.spec.scale            # (no operand of that size to combine with: the shape already differs)
    return finish(case, pre) + 0.0


# ---- the K cursor of csrc/conv.hip, restated ---------------------------------------------------------------------------------------------
def kcursor(KH, KW, Cin, CH, BK, VEC, korder):
    """(ky, kx, channel) of every K element as KCursor<CH> walks it: init(elem) for the piece at `elem` of tile 0, advance<BK> per tile.
    Returns an int64 array (K, 3) in the order the packed weight's columns are consumed."""
    K = KH * KW * Cin
    out = np.zeros((K, 3), np.int64)
    for elem in range(0, BK, VEC):
        ky = kx = 0
        if korder:
            kc, steps = elem % CH, elem // CH
        else:
            kc, steps = elem, 0

        def step(n, ky, kx, kc):
            for _ in range(n):
                kx += 1
                if kx == KW:
                    kx, kc = 0, kc + CH
                    if kc >= Cin:
                        kc, ky = kc - Cin, ky + 1
            return ky, kx, kc

        def norm(ky, kx, kc):
            while kc >= Cin:
                kc -= Cin
                kx += 1
                if kx == KW:
                    kx, ky = 0, ky + 1
            return ky, kx, kc

        ky, kx, kc = step(steps, ky, kx, kc) if korder else norm(ky, kx, kc)
        for k0 in range(elem, K, BK):
            out[k0:k0 + VEC] = np.stack([np.full(VEC, ky), np.full(VEC, kx), kc + np.arange(VEC)], 1)[:K - k0]
            ky, kx, kc = step(BK // CH, ky, kx, kc) if korder else norm(ky, kx, kc + BK)
    return out
