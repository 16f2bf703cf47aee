"""K5 (s2m2_conv2d, csrc/conv.hip) on strided, many-tap and degenerate layers against the float64 reference of tests/k5_cases.py, on every
tile id conv_select.h maps to the igemm / igemm2 families (1 - 11, 16, 17, 18, 20, 21, 22, 27) and on the heuristic (tile 0), in fp16 and
fp32, in K order 0 and -- where Cin is whole 64-byte chunks -- K order 1.  tests/test_k5_cases_cpu.py holds the same reference and
comparator against torch's own fp32 convolution and against eight wrong loaders.

  layers    3x3 s2 128 -> 128 (cnn_backbone.conv2_down.0) and 192 -> 192, 5x5 s2 16 -> 64 (conv1_down.0, K = 400) and 128 -> 128, 5x5 s1,
            1x1 s2, 3x1 / 1x3 s2, 1x7 / 7x3 s1, 1x31 s1 on W = 5, 3x3 s2 on two sources of different pixel stride, 3x3 s2 128 -> 136,
            3x3 s2 32 -> 128 on the grids on either side of the heuristic's t20_min (tile 0 only)
  shapes    (1,1,1) ... (1,33,61): k5_cases.SHAPES; every one of them on 3x3 s2 and 5x5 s2
  regimes   `exact`: small integers, the output owes every bit on every tile;  `gauss`: N(0.3, 1) activations, every element within the bound
            derived in k5_cases.bound() (NONE / RELU / GELU, out_scale 0.5, epilogues ADD / MUL / GRU / GATEMIX on the output grid)
  poison    every source is a channel slice of images 1 .. N of an (N + 2)-image buffer that is NaN everywhere else; the output is a channel
            slice of a wider tensor of sentinels with a guard image behind it, all of which must survive
  refusals  stride 3, 2x2, 5x7, and stride 2 with a halo tile, the pointwise tile, K order 2, shuffle2, ln_wsum, DUALMIX or pool2: an error,
            no launch, the output keeps its sentinel
Observed err / bound per (case, dtype, tile): profiles/k5/k5_strided.txt (S2M2_K5_STRIDED_TABLE=<path> appends the table).
"""
import os

import pytest
import torch

import k5_cases as K
from s2m2_amd import pack

pytestmark = pytest.mark.gpu
TABLE = []
F16, F32 = torch.float16, torch.float32
SENTINEL = -777.0                         # exact in fp16


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    path = os.environ.get("S2M2_K5_STRIDED_TABLE")
    if path and TABLE:
        with open(path, "a") as f:
            f.write("\n".join(TABLE) + "\n")


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == F16 else torch.int32)


def place(case, i, dtype):
    """source i on the device: the buffer (kept alive by the caller) and the view the kernel is given"""
    big = K.wide(case, i).to("cuda", dtype)
    view = big[1:1 + case.N, :, :, K.PAD:K.PAD + case.layer.cs[i]]
    assert view.stride(2) == case.layer.cs[i] + 2 * K.PAD and bool(torch.isnan(big[0]).all()) and bool(torch.isnan(big[-1]).all())
    return big, view


def guarded(n, ho, wo, cout, dtype):
    """(n, ho, wo, cout) as channels [PAD, PAD + cout) of a wider tensor of sentinels with one more image of them behind it"""
    wide = torch.full((n + 1, ho, wo, cout + 2 * K.PAD), SENTINEL, device="cuda", dtype=dtype)
    return wide, wide[:n, :, :, K.PAD:K.PAD + cout]


def intact(wide, n, cout):
    want = bits(torch.tensor([SENTINEL], device="cuda", dtype=wide.dtype))
    return (bool((bits(wide[:n, :, :, :K.PAD]) == want).all()) and bool((bits(wide[:n, :, :, K.PAD + cout:]) == want).all())
            and bool((bits(wide[n]) == want).all()))


@pytest.mark.parametrize("dt", ["float32", "float16"], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", K.NAMES)
def test_conv_vs_reference(hip, name, dt):
    case, ref = K.build(name, dt), K.reference(name, dt)
    L, spec, tdt = case.layer, case.spec, K.TDT[dt]
    placed = [place(case, i, tdt) for i in range(len(L.cs))]
    srcs = [view for _, view in placed]
    splits = [(c, c) for c in L.cs]
    bias = pack.pack_bias(case.b, L.Cout).cuda()
    a0 = None if case.a0 is None else case.a0.to("cuda", tdt)
    a1 = None if case.a1 is None else case.a1.to("cuda", tdt)
    weights = [pack.pack_conv(case.w, tdt, splits).cuda(), pack.pack_conv(case.w, tdt, splits, korder=1).cuda() if K.korder1_ok(case) else None]
    bad = []
    for tile in spec.tiles:
        results = []
        for korder, wp in enumerate(weights):
            if wp is None:
                results.append(None)
                continue
            wide, out = guarded(case.N, case.Ho, case.Wo, L.Cout, tdt)
            hip.conv2d(srcs, wp, bias, L.KH, L.KW, L.Cout, act=spec.act, epi=spec.epi, aux0=a0, aux1=a1, out=out, out_scale=spec.scale,
                       tile=tile, stride=L.stride, korder=korder)
            torch.cuda.synchronize()
            res = K.compare(case, ref, out)
            results.append(res)
            bad += [f"tile {tile} K order {korder}: {b}" for b in res.bad]
            if not intact(wide, case.N, L.Cout):
                bad.append(f"tile {tile} K order {korder}: a channel outside the output slice, or the image behind the buffer, lost its sentinel")
        TABLE.append(K.line(case, f"tile {tile:2d}  K order 0 / 1", *results))
        print(TABLE[-1])
    for (big, _), i in zip(placed, range(len(L.cs))):                   # nothing wrote into a source
        assert torch.equal(bits(big[1:1 + case.N, :, :, K.PAD:K.PAD + L.cs[i]]), bits(case.xs[i].to("cuda", tdt)))
    assert not bad, "\n".join(bad)


# ---- refusals: an error from conv2d_impl / conv_select, nothing launched ------------------------------------------------------------------
def _refusals():
    # why: (KH, KW, stride, keyword arguments, what the message says).  The layer is 128 -> 128 on (1, 8, 8).
    return {
        "stride 3": (3, 3, 3, {}, r"stride=3 \(1 or 2\)"),
        "2x2": (2, 2, 1, {}, "kernel 2x2 must be odd with at most 32 taps"),
        "5x7": (5, 7, 1, {}, "kernel 5x7 must be odd with at most 32 taps"),
        "stride 2, halo tile 12": (3, 3, 2, {"tile": 12}, "the halo tile needs a stride-1 kernel"),
        "stride 2, pointwise tile 14": (1, 1, 2, {"tile": 14}, "the pointwise kernel needs a 1x1 stride-1 layer"),
        "stride 2, K order 2": (3, 3, 2, {"korder": 2}, "K order 2 needs a stride-1|korder 2 .* is an fp16 layout"),
        "stride 2, shuffle2": (1, 1, 2, {"shuffle2": 32}, "shuffle2=32 needs a 1x1 stride-1 kernel"),
        "stride 2, ln_wsum": (1, 1, 2, {"ln_wsum": True}, "pre-LayerNorm needs a 1x1 stride-1 layer"),
        "stride 2, DUALMIX": (1, 1, 2, {"epi": 5, "act": 3, "ksplit": 64, "aux": True}, "DUALMIX needs a 1x1 stride-1 layer"),
        "stride 2, pool2": (1, 1, 2, {"pool2": True}, "pool2 needs a plain 1x1 stride-1 layer"),
    }


@pytest.mark.parametrize("dtype", [F16, F32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("why", sorted(_refusals()))
def test_refusals(hip, why, dtype):
    KH, KW, stride, kw, msg = _refusals()[why]
    kw = dict(kw)
    N, H, W, C = 1, 8, 8, 128
    x = torch.ones(N, H, W, C, device="cuda", dtype=dtype)
    w = torch.ones(C, KH * KW * C, device="cuda", dtype=dtype)
    ho, wo = -(-H // stride), -(-W // stride)
    if kw.pop("aux", False):
        kw["aux0"] = kw["aux1"] = torch.ones(N, ho, wo, C, device="cuda", dtype=dtype)
    if kw.pop("ln_wsum", False):
        kw["ln_wsum"] = torch.ones(C, device="cuda")
    shape = (N, 2 * H, 2 * W, kw["shuffle2"]) if "shuffle2" in kw else (N, ho, wo, C)      # what the binding expects of `out` for that call
    wide, out = guarded(*shape, dtype)
    with pytest.raises(RuntimeError, match=msg):
        hip.conv2d([x], w, None, KH, KW, C, out=out, stride=stride, **kw)
    torch.cuda.synchronize()
    assert bool((bits(wide) == bits(torch.tensor([SENTINEL], device="cuda", dtype=dtype))).all()), "a refused call wrote to its output"
