"""The binding's operand checks on the GPU (s2m2_amd/hip.py).  (a) A call whose operands are device tensors except ONE is refused on the
host: ValueError, and not one library entry point is called -- nothing here launches a kernel on bad input.  (b) The shared geometry
helpers hand the kernels the stride of a channel-slice view: the result equals, bit for bit, the call on the ``.contiguous()`` copy."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
C = 128


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


class _Counting:
    """stands where the loaded library would: every entry point the binding reaches for records its name and raises, so that should a
    check ever go missing, the host pointer still cannot reach a kernel"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def refuse(*args):
            self.calls.append(name)
            raise AssertionError(f"{name} was called with a host operand")
        return refuse


@pytest.fixture
def counted(hip, monkeypatch):
    proxy = _Counting()
    monkeypatch.setattr(hip, "_lib", proxy)
    return proxy


def _rand(*shape, dtype=F16, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed + len(shape) + shape[-1])
    return (torch.randn(*shape, device="cuda", generator=g) * scale).to(dtype)


def _conv2d(hip, host):
    x, w = _rand(1, 2, 8, C), _rand(C, C)
    aux = _rand(1, 2, 8, C)
    ops = dict(weight=w, bias=_rand(C, dtype=F32), ln_wsum=_rand(C, dtype=F32), bias2=_rand(C, dtype=F32))
    ops[host] = ops[host].cpu()
    hip.conv2d(x, ops["weight"], ops["bias"], 1, 1, C, epi=hip.EPI_DUALMIX, aux0=aux, aux1=aux, ln_wsum=ops["ln_wsum"], bias2=ops["bias2"],
               ksplit=64)


def _layernorm(hip, host):
    ops = dict(x=_rand(1, 2, 8, C), out=torch.empty(1, 2, 8, C, device="cuda", dtype=F16))
    ops[host] = ops[host].cpu()
    hip.layernorm(ops["x"], ops["out"])


def _mlp_chain(hip, host):
    x = _rand(1, 2, 8, C)
    hip.mlp_chain(x, [(_rand(C, C), _rand(C, dtype=F32), hip.ACT_NONE, None)], res=x.cpu(), res_stage=0)


def _feature_fusion(hip, host):
    ops = dict(z0=_rand(1, 2, 8, C), z1=_rand(1, 2, 8, C))
    ops[host] = ops[host].cpu()
    hip.feature_fusion(ops["z0"], ops["z1"], _rand(3 * C, 2 * C), _rand(3 * C, dtype=F32), _rand(C, 3 * C), _rand(C, dtype=F32), _rand(C, dtype=F32))


def _convex_upsample(hip, host):
    maps = [_rand(1, 1, 2, 8, dtype=F32)]
    hip.convex_upsample(maps, _rand(1, 8, 32, 16), 4, chan_out=torch.zeros(1, 8, 32, 8, dtype=F16)[..., 0])


REFUSED = [(_conv2d, "weight"), (_conv2d, "bias"), (_conv2d, "ln_wsum"), (_conv2d, "bias2"), (_layernorm, "x"), (_layernorm, "out"),
           (_mlp_chain, "res"), (_feature_fusion, "z0"), (_feature_fusion, "z1"), (_convex_upsample, "chan_out")]


@pytest.mark.parametrize("call,host", REFUSED, ids=[f"{c.__name__[1:]}-{h}" for c, h in REFUSED])
def test_one_host_operand_is_refused_without_a_library_call(hip, counted, call, host):
    with pytest.raises(ValueError, match="device tensors"):
        call(hip, host)
    assert counted.calls == []


def _slice_and_copy(nimg=1, seed=0):
    buf = _rand(nimg, 4, 8, 2 * C, seed=seed)
    view = buf[..., :C]
    assert not view.is_contiguous()
    return view, view.contiguous()


def _same(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    assert len(a) == len(b)
    for s, t in zip(a, b):
        assert torch.isfinite(s).all() and torch.equal(s, t)


def test_layernorm_on_a_channel_slice(hip):
    view, copy = _slice_and_copy()
    _same(hip.layernorm(view), hip.layernorm(copy))


def test_mlp_chain_on_a_channel_slice(hip):
    if not hip.mlp_chain_supported(C, F16):
        pytest.skip("no K9 at this width")
    view, copy = _slice_and_copy()
    res_view, res_copy = _slice_and_copy(seed=5)
    k = 1 / math.sqrt(C)
    stages = [(_rand(C, C, scale=k, seed=1), _rand(C, dtype=F32, seed=2), hip.ACT_GELU, None), (_rand(C, C, scale=k, seed=3), None, hip.ACT_NONE, None)]
    ln_out = (_rand(C, dtype=F32, seed=4) + 1.0, _rand(C, dtype=F32, seed=6), 1e-5) if hip.mlp_chain_ln_out_supported(C, F16) else None
    _same(hip.mlp_chain(view, stages, res=res_view, res_stage=1, ln_out=ln_out), hip.mlp_chain(copy, stages, res=res_copy, res_stage=1, ln_out=ln_out))


def test_conv_block_on_a_channel_slice(hip):
    view, copy = _slice_and_copy()
    if not hip.conv_block_supported(C, view.shape[1], view.shape[2], F16):
        pytest.skip("no K14 on this grid")
    ws = [_rand(n, scale=1 / math.sqrt(k), seed=s) for s, (n, k) in enumerate(((9 * C * C, 9 * C), (9 * C * C, 9 * C), (C * C, C), (C * C, C)))]
    bs = [_rand(C, dtype=F32, scale=0.3, seed=7 + s) for s in range(4)]
    args = (ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], ws[3], bs[3])
    _same(hip.conv_block(view, *args), hip.conv_block(copy, *args))


def test_row_attn_on_a_channel_slice(hip):
    view, copy = _slice_and_copy(nimg=2)
    if not hip.row_attn_supported(C, 1, view.shape[2], F16):
        pytest.skip("no K13 at this row width")
    weights, vectors = _rand(6 * C, C, scale=1 / math.sqrt(C), seed=1), _rand(12, C, dtype=F32, scale=0.3, seed=2)
    for cross in (False, True):
        _same(hip.row_attn(view, 1, cross, weights, vectors, ln_out_eps=1e-5), hip.row_attn(copy, 1, cross, weights, vectors, ln_out_eps=1e-5))
