"""GPU parity of K17 (s2m2_conv_gru: one ConvGRU half, reference refinenet.py:7-36, in one launch) against the two launches it replaces -- K5 v5 on
the stacked z | r layer with the r * h epilogue, K5 v5 on the candidate layer with the blend epilogue -- BIT FOR BIT on the same packed weights
(same accumulation order, same rounding points; the kernel only keeps z and r * h on the CU).
The K5 v5 kernel these bit-equalities rest on is itself held to a float64 reference on every patch form by tests/test_hip_k5_patch.py."""
import ctypes
import math

import pytest
import torch

from k5_cases import in_nan
from s2m2_amd import pack

pytestmark = pytest.mark.gpu

F16 = torch.float16
C = 128


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


_LAYERS = {}


def _layers(kh, kw):
    """(w_zr, b_zr, w_q, b_q) of one orientation, packed once: z | r stacked along Cout over cat(h, x), the candidate layer, K order 2"""
    if (kh, kw) not in _LAYERS:
        g = torch.Generator(device="cuda").manual_seed(10 * kh + kw)
        wz, wr, wq = ((torch.randn(C, 2 * C, kh, kw, device="cuda", generator=g) / math.sqrt(6 * C)).half() for _ in range(3))
        b_zr = torch.randn(2 * C, device="cuda", generator=g) * 0.3
        b_q = torch.randn(C, device="cuda", generator=g) * 0.3
        _LAYERS[(kh, kw)] = (pack.pack_conv_frag(torch.cat([wz, wr], 0), F16), b_zr, pack.pack_conv_frag(wq, F16), b_q)
    return _LAYERS[(kh, kw)]


def _inputs(N, H, W, seed, wide=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    h = torch.tanh(torch.randn(N, H, W, 3 * C if wide else C, device="cuda", generator=g) * 1.5).half()
    x = (torch.randn(N, H, W, C, device="cuda", generator=g) * 1.2 + 0.1).half()
    return (h[..., C:2 * C] if wide else h), x


def _pair(hip, h, x, kh, kw):
    """the two-launch composition of Engine.gru (the candidate layer on the 64-pixel v5 blocks, which take two epilogue operands)"""
    w_zr, b_zr, w_q, b_q = _layers(kh, kw)
    both = hip.conv2d([h, x], w_zr, b_zr, kh, kw, 2 * C, act=hip.ACT_SIGMOID, epi=hip.EPI_MUL, aux0=h, korder=2, epi_cout0=C)
    z, rh = both[..., :C], both[..., C:]
    return hip.conv2d([rh, x], w_q, b_q, kh, kw, C, act=hip.ACT_TANH, epi=hip.EPI_GRU, aux0=z, aux1=h, korder=2, tile=2)


SHAPES = [(1, 8, 20), (1, 4, 40),      # exactly one patch of the 3x1 / of the 1x3 form
          (1, 9, 44),                  # partial patches on both axes, the ring crosses all four image borders
          (2, 16, 80)]                 # several patches, two images


@pytest.mark.parametrize("taps", [(3, 1), (1, 3)], ids=["3x1", "1x3"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"n{s[0]}-{s[1]}x{s[2]}")
def test_conv_gru_equals_the_two_launches_bit_for_bit(hip, shape, taps):
    N, H, W = shape
    kh, kw = taps
    assert hip.conv_gru_supported(C, H, W, F16)
    h, x = _inputs(N, H, W, H * W)
    ref = _pair(hip, h, x, kh, kw)
    w_zr, b_zr, w_q, b_q = _layers(kh, kw)
    got = hip.conv_gru(h, x, w_zr, b_zr, w_q, b_q, kh, kw)
    assert torch.isfinite(got).all()
    assert torch.equal(got, ref), float((got.float() - ref.float()).abs().max())


@pytest.mark.parametrize("taps", [(3, 1), (1, 3)], ids=["3x1", "1x3"])
def test_conv_gru_on_a_channel_slice_and_without_biases(hip, taps):
    """h as the middle third of a 384-channel tensor (pixel stride 384); no biases"""
    kh, kw = taps
    h, x = _inputs(1, 9, 44, 7, wide=True)
    assert h.stride(2) == 3 * C and not h.is_contiguous()
    w_zr, _, w_q, _ = _layers(kh, kw)
    got = hip.conv_gru(h, x, w_zr, None, w_q, None, kh, kw)
    hc = h.contiguous()
    both = hip.conv2d([hc, x], w_zr, None, kh, kw, 2 * C, act=hip.ACT_SIGMOID, epi=hip.EPI_MUL, aux0=hc, korder=2, epi_cout0=C)
    ref = hip.conv2d([both[..., C:], x], w_q, None, kh, kw, C, act=hip.ACT_TANH, epi=hip.EPI_GRU, aux0=both[..., :C], aux1=hc, korder=2, tile=2)
    assert torch.equal(got, ref), float((got.float() - ref.float()).abs().max())


@pytest.mark.parametrize("taps", [(3, 1), (1, 3)], ids=["3x1", "1x3"])
def test_conv_gru_reads_nothing_around_its_inputs(hip, taps):
    """h and x surrounded by NaN on every side, three images (the middle one has a neighbour above and below): a ring row fetched above the
    first or below the last image, or a channel piece beside a slice, makes the output NaN"""
    kh, kw = taps
    hc, xc = _inputs(3, 9, 44, 33)
    (hbig, h), (xbig, x) = in_nan(hc), in_nan(xc)
    ref = _pair(hip, hc, xc, kh, kw)
    w_zr, b_zr, w_q, b_q = _layers(kh, kw)
    got = hip.conv_gru(h, x, w_zr, b_zr, w_q, b_q, kh, kw)
    assert torch.isfinite(got).all()
    assert torch.equal(got, ref), float((got.float() - ref.float()).abs().max())
    assert torch.equal(h, hc) and torch.equal(x, xc)
    assert int(torch.isnan(hbig).sum()) == hbig.numel() - h.numel() and int(torch.isnan(xbig).sum()) == xbig.numel() - x.numel()


def test_conv_gru_replays_from_a_plan(hip):
    kh, kw = 1, 3
    w_zr, b_zr, w_q, b_q = _layers(kh, kw)
    h, x = _inputs(1, 9, 44, 21)
    plan = hip.Plan()
    with plan.record([h, x]):
        y = hip.conv_gru(h, x, w_zr, b_zr, w_q, b_q, kh, kw)
    assert plan.launches == 1 and plan.patches(0) == 1 and plan.patches(1) == 1
    first = y.clone()
    h2, x2 = _inputs(1, 9, 44, 22)
    plan.run([h2, x2])
    assert torch.equal(y, _pair(hip, h2, x2, kh, kw)) and not torch.equal(y, first)


def test_conv_gru_refuses_what_it_does_not_take(hip):
    assert not hip.conv_gru_supported(64, 16, 16, F16) and not hip.conv_gru_supported(256, 16, 16, F16)
    assert not hip.conv_gru_supported(C, 16, 16, torch.float32)
    w_zr, b_zr, w_q, b_q = _layers(1, 3)
    h, x = _inputs(1, 4, 40, 3)
    with pytest.raises(ValueError, match="fp16"):
        hip.conv_gru(h.float(), x.float(), w_zr, b_zr, w_q, b_q, 1, 3)
    h64 = torch.zeros(1, 4, 40, 64, device="cuda", dtype=F16)
    w64 = torch.zeros(64 * 64 * 3 * 4, device="cuda", dtype=F16)
    with pytest.raises(RuntimeError, match="C=64"):
        hip.conv_gru(h64, h64.clone(), w64, None, w64[:64 * 64 * 3 * 2], None, 1, 3)
    with pytest.raises(RuntimeError, match="3 x 1 or 1 x 3"):
        _raw(hip, h, x, w_zr, w_q, KH=1, KW=1)
    with pytest.raises(RuntimeError, match="x is null"):
        _raw(hip, h, None, w_zr, w_q)
    with pytest.raises(RuntimeError, match="w_q is null"):
        _raw(hip, h, x, w_zr, None)
    with pytest.raises(RuntimeError, match="out aliases h"):
        _raw(hip, h, x, w_zr, w_q, out=h)


def _raw(hip, h, x, w_zr, w_q, KH=1, KW=3, out=None):
    """the C entry with a descriptor of our own (what the wrapper never builds: a null operand, an aliased output, a 1x1 layer)"""
    d = hip.ConvGruDesc()
    o = torch.empty_like(h) if out is None else out
    d.h, d.h_stride, d.x, d.x_stride, d.out, d.out_stride = h.data_ptr(), C, (x.data_ptr() if x is not None else None), C, o.data_ptr(), C
    d.N, d.H, d.W, d.C, d.KH, d.KW = 1, h.shape[1], h.shape[2], C, KH, KW
    d.w_zr, d.w_q, d.dtype = w_zr.data_ptr(), (w_q.data_ptr() if w_q is not None else None), hip.F16
    rc = hip.load().s2m2_conv_gru(ctypes.byref(d), None)
    if rc != 0:
        raise RuntimeError(hip.load().s2m2_last_error().decode())
    return o
