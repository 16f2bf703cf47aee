"""GPU checks of the row -> (n, y, x) walk (s2m2_amd/csrc/row_coord.h) inside the kernels that use it, by EXACT equality against the
unfused path, where the same pixels are addressed by a stand-alone kernel or by the host:
  * K10 with the coarse z1 read through the x2 resampling   ==  K7 resample2x, then K10 on the full-size tensor;
  * K9 with AvgPool2d(2) folded into its tile load          ==  K7's pooling kernel, then K9;
  * K11's pixel-shuffle store                               ==  K11's plain store, permuted on the host.
The shapes are the small ones at which the walk can go wrong: image rows shorter than the distance between a thread's pieces (16 rows in
K10 / K9, 16 - 64 in K11), so that one step carries over several image rows or whole images; tiles that straddle images; a ragged last tile;
and the 64-row form of K10 one shape above each of its thresholds."""
import math

import pytest
import torch

from s2m2_amd import pack

pytestmark = pytest.mark.gpu

DT = torch.float16


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


_FUSION_W = {}


def _fusion_weights(C):
    """(LDS-form arguments, direct-form arguments) of one FeatureFusion of width C, made once per width"""
    if C not in _FUSION_W:
        g = torch.Generator(device="cuda").manual_seed(3 * C)
        w1 = (torch.randn(3 * C, 2 * C, 1, 1, device="cuda", generator=g) / math.sqrt(2 * C)).to(DT)
        wg = (torch.randn(C, C, 1, 1, device="cuda", generator=g) / math.sqrt(C)).to(DT)
        wf = (torch.randn(C, 2 * C, 1, 1, device="cuda", generator=g) / math.sqrt(2 * C)).to(DT)
        b1, bg, bf = (pack.pack_bias(torch.randn(n, device="cuda", generator=g) * 0.5, n) for n in (3 * C, C, C))
        p1 = pack.pack_conv(w1, DT)
        p2 = torch.cat([pack.pack_conv(wg, DT), pack.pack_conv(wf, DT)], dim=1).contiguous()
        _FUSION_W[C] = ((p1, b1, p2, bg, bf), (pack.fusion_frag(p1, p2), b1, None, bg, bf))
    return _FUSION_W[C]


def _k10_case(hip, C, coarse_shape, strided=False):
    n, h, w = coarse_shape
    g = torch.Generator(device="cuda").manual_seed(C + 31 * h + w)
    wide = torch.randn(n, 2 * h, 2 * w, C + 8, device="cuda", generator=g).to(DT)
    z0 = wide[..., :C] if strided else wide[..., :C].contiguous()
    zc = (torch.randn(n, h, w, C, device="cuda", generator=g) * 1.5).to(DT)
    up = hip.resample2x(zc, 1)                                      # K7: the stand-alone x2 resampling
    lds, direct = _fusion_weights(C)
    for args, kw in ((direct, {"frag": True}), (lds, {})):
        fused = hip.feature_fusion(z0, zc, *args, z1_coarse=True, **kw)
        unfused = hip.feature_fusion(z0, up, *args, **kw)
        assert fused.shape == unfused.shape and torch.equal(fused, unfused), (kw, int((fused != unfused).sum()))


@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("shape", [(2, 1, 1), (2, 3, 5), (3, 5, 1), (1, 7, 19)])
def test_k10_coarse_shapes(hip, C, shape):
    """fine rows of 2 / 10 / 2 / 38 pixels against a 16-row step: tiles straddle image rows and images, one step wraps several image rows"""
    _k10_case(hip, C, shape)


@pytest.mark.parametrize("C", [128, 256])
def test_k10_tail_tile(hip, C):
    """6 x 14 = 84 fine rows: two full 32-row tiles and one of 20 rows (strided z0 rows as well)"""
    assert (2 * 3 * 2 * 7) % 32 != 0
    _k10_case(hip, C, (1, 3, 7), strided=True)


@pytest.mark.parametrize("C,shape", [(128, (2, 64, 100)), (256, (2, 34, 38))])
def test_k10_tall_form(hip, C, shape):
    """one shape above each threshold of the 64-row form of the direct kernel (24576 rows at C = 128, 8192 at C = 256)"""
    n, h, w = shape
    assert n * 4 * h * w > (24576 if C == 128 else 8192)
    _k10_case(hip, C, shape)


@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("shape", [(2, 6, 10), (1, 2, 38)])
def test_k9_pool_odd_pooled_widths(hip, C, shape):
    """pooled grids of 3 x 5 and 1 x 19 pixels: K9 with the pooling folded into its tile load == K7's pooling kernel, then K9"""
    n, h, w = shape
    g = torch.Generator(device="cuda").manual_seed(C + h)
    wide = torch.randn(n, h, w, C + 8, device="cuda", generator=g).to(DT)
    x = wide[..., :C]                                               # strided pixels
    stages = []
    for i in range(2):
        wq = (torch.randn(C, C, 1, 1, device="cuda", generator=g) / math.sqrt(C)).to(DT)
        b = pack.pack_bias(torch.randn(C, device="cuda", generator=g) * 0.3, C)
        stages.append((pack.chain_frag(pack.pack_conv(wq, DT)), b, hip.ACT_GELU if i == 0 else hip.ACT_NONE, None))
    pooled = hip.resample2x(x.contiguous(), 0)
    fused = hip.mlp_chain(x, stages, frag=True, pool2=True)
    unfused = hip.mlp_chain(pooled, stages, frag=True)
    assert tuple(fused.shape) == (n, h // 2, w // 2, C) and torch.equal(fused, unfused)
    wfan = pack.pack_conv((torch.randn(2 * C, C, 1, 1, device="cuda", generator=g) / math.sqrt(C)).to(DT), DT)
    bfan = pack.pack_bias(torch.randn(2 * C, device="cuda", generator=g) * 0.3, 2 * C)
    assert torch.equal(hip.mlp_fan(x, pack.chain_frag(wfan), bfan, None, frag=True, pool2=True), hip.mlp_fan(pooled, pack.chain_frag(wfan), bfan, None, frag=True))


@pytest.mark.parametrize("cin,cout", [(128, 64), (128, 16), (128, 9)])
@pytest.mark.parametrize("shape", [(2, 3, 5), (1, 5, 1)])
def test_k11_shuffle2_store(hip, cin, cout, shape):
    """ConvTranspose2d(2, stride 2) store: cout (dy * 2 + dx) * C' + c' of input pixel (n, y, x) -> channel c' of output pixel (n, 2y + dy, 2x + dx)"""
    n, h, w = shape
    g = torch.Generator(device="cuda").manual_seed(cin + cout + h)
    x = (torch.randn(n, h, w, cin, device="cuda", generator=g) * 1.2).to(DT)
    wt = (torch.randn(cin, cout, 2, 2, device="cuda", generator=g) / math.sqrt(cin)).to(DT)
    wp, cp = pack.pack_convT_2x2s2(wt, DT)
    bp = pack.pack_bias_shuffle(torch.randn(cout, device="cuda", generator=g) * 0.3, cout)
    assert hip.pw_direct_supported(cin, 4 * cp, DT)
    wf = pack.pw_frag(wp)
    shuffled = hip.pw_direct([x], wf, bp, 4 * cp, shuffle2=cp)
    plain = hip.pw_direct([x], wf, bp, 4 * cp)
    assert tuple(plain.shape) == (n, h, w, 4 * cp) and tuple(shuffled.shape) == (n, 2 * h, 2 * w, cp)
    host = plain.reshape(n, h, w, 2, 2, cp).permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * h, 2 * w, cp)
    assert torch.equal(shuffled, host)
