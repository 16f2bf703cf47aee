"""GPU parity of K19 (s2m2_conv_block_tail: the second half of a ConvBlock2D, reference attentions.py:255-281, in one launch) against the two
launches it replaces -- the K9 two-stage chain on the 1x1 branch, K5 v5 on convs.2 with the residual epilogue -- BIT FOR BIT on the same packed
weights (same accumulation order, same rounding points; the kernel only keeps the 1x1 branch's output on the CU), and the whole forward with the
path switched on and off.
The K5 v5 kernel these bit-equalities rest on is itself held to a float64 reference on every patch form by tests/test_hip_k5_patch.py."""
import ctypes
import math

import pytest
import torch

from k5_cases import in_nan
from s2m2_amd import pack

pytestmark = pytest.mark.gpu

F16 = torch.float16


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


_LAYERS = {}


def _layers(C):
    """(w_conv2, a0, a2, [b_conv2, b_1x0, b_1x2]) of one width, packed once: the 3x3 layer in K order 2, the 1x1 layers in K9's fragment order"""
    if C not in _LAYERS:
        g = torch.Generator(device="cuda").manual_seed(C)
        k2 = (torch.randn(C, C, 3, 3, device="cuda", generator=g) / math.sqrt(9 * C)).half()
        p0 = (torch.randn(C, C, 1, 1, device="cuda", generator=g) / math.sqrt(C)).half()
        p2 = (torch.randn(C, C, 1, 1, device="cuda", generator=g) / math.sqrt(C)).half()
        bs = [torch.randn(C, device="cuda", generator=g) * 0.3 for _ in range(3)]
        _LAYERS[C] = (pack.pack_conv_frag(k2, F16), pack.chain_frag(pack.pack_conv(p0, F16)), pack.chain_frag(pack.pack_conv(p2, F16)), bs)
    return _LAYERS[C]


def _inputs(N, H, W, C, seed, wide=False):
    """t like a GELU output, z like a feature map; wide: both as the middle third of a tensor three times as wide"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    cw = 3 * C if wide else C
    t = torch.nn.functional.gelu(torch.randn(N, H, W, cw, device="cuda", generator=g) * 1.2).half()
    z = (torch.randn(N, H, W, cw, device="cuda", generator=g) * 1.3 + 0.2).half()
    return (t[..., C:2 * C], z[..., C:2 * C]) if wide else (t, z)


def _pair(hip, t, z, bias=True):
    """the two-launch composition of Engine.conv_block"""
    C = t.shape[-1]
    w2, a0, a2, bs = _layers(C)
    b2, ba, bb = bs if bias else (None, None, None)
    b = hip.mlp_chain(z, [(a0, ba, hip.ACT_RELU, None), (a2, bb, hip.ACT_NONE, None)], frag=True)
    return hip.conv2d([t], w2, b2, 3, 3, C, epi=hip.EPI_ADD, aux0=b, korder=2)


def _tail(hip, t, z, bias=True, **kw):
    w2, a0, a2, bs = _layers(t.shape[-1])
    b2, ba, bb = bs if bias else (None, None, None)
    return hip.conv_block_tail(t, z, w2, b2, a0, ba, a2, bb, **kw)


CASES = [  # N, H, W, C, patch
    (1, 4, 40, 128, (4, 40)), (1, 4, 32, 128, (4, 32)), (1, 2, 32, 128, (2, 32)),      # exactly one patch of each form
    (1, 5, 41, 128, (4, 40)), (1, 5, 41, 128, (4, 32)), (1, 5, 41, 128, (2, 32)),      # partial patches on both axes: the halo crosses all four borders
    (2, 9, 70, 128, (4, 40)), (2, 9, 70, 128, None),                                   # several patches, two images
    (1, 1, 1, 128, None), (1, 1, 1, 128, (4, 40)),
    (1, 2, 32, 256, (2, 32)), (1, 3, 33, 256, None), (1, 3, 33, 256, (4, 40)),          # two channel chunks, eight waves
    (2, 5, 70, 256, None), (2, 5, 70, 256, (4, 32)), (2, 5, 70, 256, (4, 40)),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"n{c[0]}-{c[1]}x{c[2]}-C{c[3]}-p{'x'.join(map(str, c[4])) if c[4] else 'auto'}")
def test_conv_block_tail_equals_the_two_launches_bit_for_bit(hip, case):
    N, H, W, C, patch = case
    assert hip.conv_block_tail_supported(C, H, W, F16)
    t, z = _inputs(N, H, W, C, H * W + C)
    ref = _pair(hip, t, z)
    got = _tail(hip, t, z, patch=patch)
    assert torch.isfinite(got).all()
    assert torch.equal(got, ref), float((got.float() - ref.float()).abs().max())


@pytest.mark.parametrize("C", [128, 256])
def test_conv_block_tail_on_channel_slices_into_a_strided_output_without_biases(hip, C):
    """t and z as the middle third of tensors three times as wide (pixel stride 3C), out with a pixel stride above C, no biases"""
    t, z = _inputs(1, 5, 41, C, 7, wide=True)
    assert t.stride(2) == 3 * C and not t.is_contiguous() and not z.is_contiguous()
    ref = _pair(hip, t.contiguous(), z.contiguous(), bias=False)
    buf = torch.full((1, 5, 41, C + 64), 7.0, device="cuda", dtype=F16)
    out = buf[..., 8:8 + C]
    got = _tail(hip, t, z, bias=False, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(out, ref), float((out.float() - ref.float()).abs().max())
    assert bool((buf[..., :8] == 7.0).all()) and bool((buf[..., 8 + C:] == 7.0).all())          # nothing written beside the view


@pytest.mark.parametrize("C,patch", [(128, (2, 32)), (128, (4, 32)), (128, (4, 40)), (256, None)],
                         ids=["C128-p2x32", "C128-p4x32", "C128-p4x40", "C256-auto"])
def test_conv_block_tail_reads_and_writes_nothing_around_its_operands(hip, C, patch):
    """t and z surrounded by NaN on every side, three images (the middle one has a neighbour above and below), the output a channel slice of a
    tensor of sentinels with a guard image behind it: a halo row fetched above the first or below the last image, or a channel piece beside a
    slice, makes the output NaN; a store beside the slice or behind the last image loses a sentinel"""
    N, H, W = 3, 5, 41
    tc, zc = _inputs(N, H, W, C, 77 + C)
    (tbig, t), (zbig, z) = in_nan(tc), in_nan(zc)
    ref = _pair(hip, tc, zc)
    sentinel = torch.tensor(-777.0, device="cuda", dtype=F16)
    buf = torch.full((N + 1, H, W, C + 16), -777.0, device="cuda", dtype=F16)
    out = buf[:N, :, :, 8:8 + C]
    got = _tail(hip, t, z, out=out, patch=patch)
    assert got.data_ptr() == out.data_ptr() and torch.isfinite(out).all()
    assert torch.equal(out, ref), float((out.float() - ref.float()).abs().max())
    assert bool((buf[:N, :, :, :8] == sentinel).all()) and bool((buf[:N, :, :, 8 + C:] == sentinel).all()) and bool((buf[N] == sentinel).all())
    assert torch.equal(t, tc) and torch.equal(z, zc)
    assert int(torch.isnan(tbig).sum()) == tbig.numel() - t.numel() and int(torch.isnan(zbig).sum()) == zbig.numel() - z.numel()


def test_conv_block_tail_replays_from_a_plan(hip):
    t, z = _inputs(1, 5, 41, 128, 21)
    plan = hip.Plan()
    with plan.record([t, z]):
        y = _tail(hip, t, z)
    assert plan.launches == 1 and plan.patches(0) == 1 and plan.patches(1) == 1
    first = y.clone()
    t2, z2 = _inputs(1, 5, 41, 128, 22)
    plan.run([t2, z2])
    assert torch.equal(y, _pair(hip, t2, z2)) and not torch.equal(y, first)


def _raw(hip, t_in, z_in, out_t=None, **kw):
    """the C entry with a descriptor of our own (what the wrapper never builds: a null operand, an aliased output, a bad stride)"""
    w2, a0, a2, _ = _layers(128)
    d = hip.ConvTailDesc()
    o = torch.empty(t_in.shape, device="cuda", dtype=F16) if out_t is None else out_t
    C = 128
    d.t, d.t_stride, d.z, d.z_stride, d.out, d.out_stride = t_in.data_ptr(), C, z_in.data_ptr(), C, o.data_ptr(), C
    d.N, d.H, d.W, d.C = 1, t_in.shape[1], t_in.shape[2], C
    d.w_conv2, d.w_1x0, d.w_1x2, d.dtype = w2.data_ptr(), a0.data_ptr(), a2.data_ptr(), hip.F16
    for k, v in kw.items():
        setattr(d, k, v)
    rc = hip.load().s2m2_conv_block_tail(ctypes.byref(d), None)
    if rc != 0:
        raise RuntimeError(hip.load().s2m2_last_error().decode())
    return o


def test_conv_block_tail_refuses_what_it_does_not_take(hip):
    assert not hip.conv_block_tail_supported(64, 16, 16, F16) and not hip.conv_block_tail_supported(192, 16, 16, F16)
    assert not hip.conv_block_tail_supported(128, 16, 16, torch.float32) and not hip.conv_block_tail_supported(256, 16, 16, torch.float32)
    t, z = _inputs(1, 4, 40, 128, 3)
    for kw, msg in (({"t": None}, "t is null"), ({"z": None}, "z is null"), ({"out": None}, "out is null"), ({"w_conv2": None}, "w_conv2 is null"),
                    ({"w_1x0": None}, "w_1x0 is null"), ({"w_1x2": None}, "w_1x2 is null"), ({"dtype": hip.F32}, "fp16 only"),
                    ({"C": 64}, "C=64"), ({"C": 192}, "C=192"), ({"t_stride": 132}, "t_stride=132"), ({"z_stride": 140}, "z_stride=140"),
                    ({"out_stride": 129}, "out_stride=129"), ({"patch_rows": 2, "patch_cols": 40}, "patch 2 x 40")):
        with pytest.raises(RuntimeError, match=msg):
            _raw(hip, t, z, **kw)
    with pytest.raises(RuntimeError, match="out aliases t"):
        _raw(hip, t, z, out_t=t)
    with pytest.raises(RuntimeError, match="out aliases z"):
        _raw(hip, t, z, out_t=z)
    with pytest.raises(ValueError, match="fp16"):
        _tail(hip, t.float(), z.float())


# ---- the whole forward, S model, 64 x 96, refine_iter 1, with the path on and off in one process

def _forward_and_count(hip, monkeypatch, switch, use_convblock):
    from s2m2_amd.model import S2M2
    from s2m2_amd.spec import MODEL_CONFIGS
    from s2m2_amd.weights import seeded_state_dict, synthetic_pair
    monkeypatch.setenv("S2M2_CB_TAIL", switch)
    C, ntr = MODEL_CONFIGS["S"]
    m = S2M2(C, 1, ntr, use_positivity=True, output_upsample=False, refine_iter=1)
    m.load_state_dict(seeded_state_dict(C, 1, ntr, 0), strict=True)
    m = m.cuda().eval()
    left, right = (x.cuda().contiguous() for x in synthetic_pair(64, 96, 1, 24, 0))
    eng = m.engine(F16)
    assert eng.cb_tail == (switch == "1")
    eng.use_convblock = use_convblock
    eng.cb_tail_c256 = True                                       # off by default (no gain at the 1/16 level); the forward must be right with it too
    with torch.no_grad(), torch.autocast("cuda", dtype=F16):
        for _ in range(3):                                       # eager, graph capture (the refiner's recorded plans inside), replay
            outs = [o.clone() for o in m(left, right)]
    hip.METER = {}
    try:
        with torch.no_grad(), torch.autocast("cuda", enabled=False):
            eng.run(left, right, None)
        torch.cuda.synchronize()
        meter = hip.METER
    finally:
        hip.METER = None
    return outs, sum(v[1] for v in meter.values()), meter.get("conv_block_tail", [0.0, 0])[1]


@pytest.mark.parametrize("use_convblock", [True, False], ids=["k14-on", "k14-off"])
def test_forward_is_bit_identical_with_the_path_on_and_off(hip, monkeypatch, use_convblock):
    """With K19 enabled at C = 256 as well.  K14 on: only the C = 256 blocks take K19 at this size; K14 off: the C = 128 blocks too.  One launch
    less per block that switched."""
    off, n_off, tails_off = _forward_and_count(hip, monkeypatch, "0", use_convblock)
    on, n_on, tails_on = _forward_and_count(hip, monkeypatch, "1", use_convblock)
    assert tails_off == 0 and tails_on > 0
    assert n_off - n_on == tails_on, (n_off, n_on, tails_on)
    for a, b, name in zip(on, off, ("disp", "occ", "conf")):
        assert a.shape == b.shape and torch.equal(a, b), name
