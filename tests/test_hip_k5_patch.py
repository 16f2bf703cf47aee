"""K5 (s2m2_conv2d, csrc/conv.hip) on stride-1 3x3, 3x1 and 1x3 layers against the float64 reference of tests/k5_cases.py, on the two kernel
families that carry them in the forward: the v3 halo tiles (tile ids 12, 13, 19, 23, 24, 25, 26 and the heuristic's own pick, K order 0, fp16
and fp32) and the v5 fragment-stream kernel (K order 2, fp16: 2x32, 4x32 and 4x40 pixel patches and the selector's own pick, on blocks of 128
and of 192 output channels).  The fragment-stream kernel is what K14, K17 and K19 are held bit-equal to (tests/test_hip_convblock.py,
tests/test_hip_conv_gru.py, tests/test_hip_convtail.py): this is where it meets a float64 reference itself.  tests/k5_patch_cases.py lists the
layers, shapes, regimes and launches; tests/test_k5_patch_cases_cpu.py holds the same reference and comparator against torch's own fp32
convolution and against twelve wrong patch loaders.

  poison    every source and every epilogue operand is a channel slice of images 1 .. N of an (N + 2)-image buffer that is NaN everywhere else;
            the output is a channel slice of a wider tensor of sentinels with a guard image behind it.  After every launch the sentinels must be
            intact and the sources unchanged
  regimes   `exact`: the output owes every bit, and +0.0 for zero, on every launch;  `gauss`: every element within k5_cases.bound()
  refusals  a two-operand epilogue (GRU, GATEMIX) on the 128- and 160-pixel blocks (tile 4, tile 40): an error, no launch, the output keeps its
            sentinel.  k5_patch_cases.launches() leaves exactly these out
  launches  every launch is also run through csrc/conv_select.h on the host (k5_patch_cases.selection()): a forced tile must select the form it
            names, and a line of the table names the kernel that ran ("frag 128 128 4 40 0": cout block, chunk, PH, PW, operands), not the request
Observed err / bound per (case, dtype, launch): profiles/k5/k5_patch.txt (S2M2_K5_PATCH_TABLE=<path> appends the table).
"""
import os

import pytest
import torch

import k5_cases as K
import k5_patch_cases as P
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
    path = os.environ.get("S2M2_K5_PATCH_TABLE")
    if path and TABLE:
        with open(path, "a") as f:
            f.write("\n".join(TABLE) + "\n")


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == F16 else torch.int32)


def place(t, dtype):
    """an (N, H, W, c) operand on the device: the NaN-surrounded buffer (kept alive by the caller) and the view the kernel is given"""
    N, c = t.shape[0], t.shape[-1]
    big = K.widen(t).to("cuda", dtype)
    view = big[1:1 + N, :, :, K.PAD:K.PAD + c]
    assert view.stride(2) == c + 2 * K.PAD and bool(torch.isnan(big[0]).all()) and bool(torch.isnan(big[-1]).all())
    return big, view


def guarded(n, ho, wo, cout, dtype):
    """(n, ho, wo, cout) as channels [PAD, PAD + cout) of a wider tensor of sentinels with one more image of them behind it"""
    wide = torch.full((n + 1, ho, wo, cout + 2 * K.PAD), SENTINEL, device="cuda", dtype=dtype)
    return wide, wide[:n, :, :, K.PAD:K.PAD + cout]


def intact(wide, n, cout):
    want = bits(torch.tensor([SENTINEL], device="cuda", dtype=wide.dtype))
    return (bool((bits(wide[:n, :, :, :K.PAD]) == want).all()) and bool((bits(wide[:n, :, :, K.PAD + cout:]) == want).all())
            and bool((bits(wide[n]) == want).all()))


# (an epi_cout0 case has no fp32 launch: K order 2 is an fp16 layout)
RUNS = [(n, dt) for n in P.NAMES for dt in ("float32", "float16") if P.SPECS[n].halo or dt == "float16"]


@pytest.mark.parametrize("name,dt", RUNS, ids=[f"{n}-{K.SHORT[dt]}" for n, dt in RUNS])
def test_conv_vs_reference(hip, name, dt):
    case, ref = P.build(name, dt), P.reference(name, dt)
    L, spec, tdt = case.layer, case.spec, K.TDT[dt]
    todo = P.launches(case)
    assert todo
    operands = [t for t in case.xs + (case.a0, case.a1) if t is not None]
    placed = [place(t, tdt) for t in operands]
    srcs = [view for _, view in placed[:len(L.cs)]]
    aux = [view for _, view in placed[len(L.cs):]] + [None, None]
    splits = [(c, c) for c in L.cs]
    bias = pack.pack_bias(case.b, L.Cout).cuda()
    weights = {0: pack.pack_conv(case.w, tdt, splits).cuda()}
    if any(l.korder == 2 for l in todo):
        weights[2] = pack.pack_conv_frag(case.w, tdt, splits).cuda()
    bad = []
    for l in todo:
        what = P.label(case, l)                                          # the request and the kernel conv_select.h chooses for it
        assert P.forced(case, l) in (None, P.chosen(case, l)), f"{what}: a forced tile must run the form it names"
        wide, out = guarded(case.N, case.H, case.W, L.Cout, tdt)
        hip.conv2d(srcs, weights[l.korder], bias, L.KH, L.KW, L.Cout, act=spec.act, epi=spec.epi, aux0=aux[0], aux1=aux[1], out=out,
                   out_scale=spec.scale, tile=l.tile, korder=l.korder, epi_cout0=spec.epi_cout0)
        torch.cuda.synchronize()
        res = K.compare(case, ref, out)
        bad += [f"{what}: {b}" for b in res.bad]
        if not intact(wide, case.N, L.Cout):
            bad.append(f"{what}: a channel outside the output slice, or the image behind the buffer, lost its sentinel")
        TABLE.append(K.line(case, what, res))
        print(TABLE[-1])
    for (big, _), t in zip(placed, operands):                            # nothing wrote into a source or an operand
        assert torch.equal(bits(big[1:1 + case.N, :, :, K.PAD:K.PAD + t.shape[-1]]), bits(t.to("cuda", tdt)))
    assert not bad, "\n".join(bad)


# ---- refusals: an error from conv_select_frag, nothing launched ---------------------------------------------------------------------------
@pytest.mark.parametrize("C", [128, 192], ids=["cb128", "cb192"])
@pytest.mark.parametrize("epi,tile", P.REFUSED, ids=[f"{K.EPI_NAME[e]}-tile{t}" for e, t in P.REFUSED])
def test_refusals(hip, epi, tile, C):
    N, H, W = 1, 4, 40
    x = torch.ones(N, H, W, C, device="cuda", dtype=F16)
    w = torch.ones(C, 3 * C, device="cuda", dtype=F16)
    a = torch.ones(N, H, W, C, device="cuda", dtype=F16)
    wide, out = guarded(N, H, W, C, F16)
    with pytest.raises(RuntimeError, match="takes one-operand epilogues only"):
        hip.conv2d([x], w, None, 1, 3, C, epi=epi, aux0=a, aux1=a, out=out, korder=2, tile=tile)
    torch.cuda.synchronize()
    assert bool((bits(wide) == bits(torch.tensor([SENTINEL], device="cuda", dtype=F16))).all()), "a refused call wrote to its output"
    hip.conv2d([x], w, None, 1, 3, C, epi=epi, aux0=a, aux1=a, out=out, korder=2, tile=2)      # the 64-pixel blocks take it
    torch.cuda.synchronize()
    assert intact(wide, N, C) and not bool((out == SENTINEL).any())
