"""The power of tests/module_parity.py's ``judge`` (no GPU): the oracle's own fp16 emulation must pass it, and a mutated oracle -- run in the
same fp16 emulation, on the shapes of the GPU cases (a few rows at full width) -- must fail it, for every mutation below.  Each mutation is
a bug a fused kernel or its weight packing could plausibly have and that a self-consistent restatement would share.

Measured on the two mutations the issue asked to measure (ratios of the mutant's error to the emulation's, median / p99 / max, and the
fractions of elements beyond 4 fp16 ulps), BasicAttnBlock at w = 304:

* one intermediate (the FFN hidden tensor) rounded to bf16 instead of fp16: rejected -- 2.9x / 2.5x / 1.95x, 31 % vs 9.7 % beyond 4 ulps;
* GELU in its tanh form: rejected only by a hair, by the ulp count alone (10.0 % vs 9.7 %) -- 1.05x / 1.02x / 1.00x.  The tanh form is within
  ~3e-4 of the erf form, below an fp16 ulp of most of the hidden tensor: close to a blind spot of a comparator built on the emulation's
  spread (tests/test_gelu16_cpu.py pins the kernels' GELU itself).
"""
import pytest
import torch
import torch.nn.functional as F

import module_parity as MP
from oracle import s2m2_oracle as O
from s2m2_amd.weights import seeded_state_dict

MRT = "transformer.uformer_list.0"


@pytest.fixture(scope="module")
def sd():
    return MP.sd16(seeded_state_dict(128, 1, 1, 0))


def _basic(sd, block, nh, w, rows=2, seed=0):
    z = MP.seeded((2, sd[block + ".ffn.ffn.0.weight"].shape[1], rows, w), seed)
    fn = lambda: MP.nhwc(O.basic_attn_block(sd, block, z, nh))          # noqa: E731
    return fn


def _global_pe(sd, block, h=32, w=38, seed=1):
    c = sd[block + ".ffn.ffn.0.weight"].shape[1]
    z = MP.seeded((2, c, h, w), seed)
    return lambda: MP.nhwc(O.global_attn_block(sd, block, z, 8, O.dense_pe(h, w)))      # noqa: E731


def _conv_block(sd, block, w=304, rows=4, seed=2):
    z = MP.seeded((2, sd[block + ".convs.0.weight"].shape[1], rows, w), seed)
    return lambda: MP.nhwc(O.conv_block(sd, block, z))                                  # noqa: E731


def _run(fn, mutation=None):
    """(y32, y16e, the mutated module in the fp16 emulation)"""
    y32, y16e = MP.oracle_pair(fn)
    if mutation is None:
        return y32, y16e, None
    with mutation(), torch.no_grad(), O.precision("fp16"):
        ym = fn()
    return y32, y16e, ym


def _sdpa_mut(edit):
    """O._sdpa with its inputs / output edited: edit(q, k, v) -> (q, k, v, post) where post(o) edits the output"""
    real = O._sdpa

    def sdpa(q, k, v, explicit=False):
        q, k, v, post = edit(q, k, v)
        o, a = real(q, k, v, explicit)
        return post(o), a
    return lambda: MP.patched(O, "_sdpa", sdpa)


def _same(o):
    return o


def _own_view():
    def cross(sd, p, x, y, nh):              # keys / values from the query's own view: the halves are not swapped
        return O.self_attn(sd, p, x, nh, None), O.self_attn(sd, p, y, nh, None)
    return MP.patched(O, "cross_attn", cross)


def _shift_second_chunk(q, k, v):            # keys 160.. (the second chunk of 160) read one token late; the last key twice
    if k.shape[-2] == 304:
        k = torch.cat([k[..., :160, :], k[..., 161:, :], k[..., -1:, :]], -2)
    return q, k, v, _same


def _drop_last_tile(q, k, v):                # no attention output for the last partial 32-token tile (tokens 288..299)
    def post(o):
        if o.shape[-2] == 300:
            o = o.clone()
            o[..., 288:, :] = 0
        return o
    return q, k, v, post


def _swap_head_v(q, k, v):                   # head 0 reads head 1's V and vice versa
    if v.shape[1] == 2:
        v = v.flip(1)
    return q, k, v, _same


def _replicate_right_edge():
    real = O._conv

    def conv(sd, p, x, stride=1, pad=0):
        if p.endswith(".convs.0") and pad == 1:
            w, b = O._wb(sd, p)
            xp = F.pad(O._q(x), (1, 0, 1, 1))
            xp = torch.cat([xp, xp[..., -1:]], -1)                   # right edge replicated instead of zero
            return O._q(F.conv2d(xp, w, b))
        return real(sd, p, x, stride, pad)
    return MP.patched(O, "_conv", conv)


def _transposed_pe():
    real = O.dense_pe
    return MP.patched(O, "dense_pe", lambda h, w, pe_dim=32: real(h, w, pe_dim).transpose(0, 1).contiguous())


def _gelu_bf16_hidden():
    real = O._lin

    def lin(sd, p, x):
        y = real(sd, p, x)
        return y.bfloat16().float() if p.endswith(".ffn.0") else y      # the FFN hidden tensor (pre-GELU) rounded to bf16
    return MP.patched(O, "_lin", lin)


def _gelu_tanh():
    return MP.patched(O, "_gelu", lambda x: O._q(F.gelu(x, approximate="tanh")))


CASES = {
    # id: (module under test, mutation)
    "cross_attends_own_view": (lambda sd: _basic(sd, MRT + ".enc_attn0", 1, 304), _own_view),
    "second_key_chunk_shifted_w304": (lambda sd: _basic(sd, MRT + ".enc_attn0", 1, 304), _sdpa_mut(_shift_second_chunk)),
    "last_partial_tile_dropped_w300": (lambda sd: _basic(sd, MRT + ".enc_attn0", 1, 300), _sdpa_mut(_drop_last_tile)),
    "heads_swap_v_2heads": (lambda sd: _basic(sd, MRT + ".enc_attn1", 2, 152), _sdpa_mut(_swap_head_v)),
    "convblock_right_edge_replicated": (lambda sd: _conv_block(sd, "feat_pyramid.enc0"), _replicate_right_edge),
    "pe_table_transposed": (lambda sd: _global_pe(sd, "feat_pyramid.enc3s.0"), _transposed_pe),
}


@pytest.mark.parametrize("name", list(CASES))
def test_judge_rejects_mutation(sd, name):
    build, mutation = CASES[name]
    y32, y16e, ym = _run(build(sd), mutation)
    assert MP.judge(y16e, y32, y16e, "emulation").ok, MP.judge(y16e, y32, y16e, "emulation").msg
    v = MP.judge(ym, y32, y16e, name)
    assert not v.ok, f"{name} passed the comparator: {v.row()}"


@pytest.mark.parametrize("name,build", [("basic_w304", lambda sd: _basic(sd, MRT + ".enc_attn0", 1, 304)),
                                        ("basic_2heads_w152", lambda sd: _basic(sd, MRT + ".enc_attn1", 2, 152)),
                                        ("global_pe", lambda sd: _global_pe(sd, "feat_pyramid.enc3s.0")),
                                        ("convblock", lambda sd: _conv_block(sd, "feat_pyramid.enc0"))])
def test_judge_accepts_the_emulation(sd, name, build):
    y32, y16e, _ = _run(build(sd))
    v = MP.judge(y16e, y32, y16e, name)
    assert v.ok, v.msg
    assert v.emu["max"] > 0                      # the yardstick is not degenerate


@pytest.mark.parametrize("name,mutation,rejected", [("bf16_hidden", _gelu_bf16_hidden, True), ("gelu_tanh", _gelu_tanh, True)])
def test_judge_measured_mutations(sd, name, mutation, rejected):
    """the two measured mutations (module docstring): the outcome is pinned both ways, so that a change of the comparator that makes
    the blind spot visible (or loses the bf16 case) is noticed and the docstring updated"""
    y32, y16e, ym = _run(_basic(sd, MRT + ".enc_attn0", 1, 304), mutation)
    v = MP.judge(ym, y32, y16e, name)
    print(name, v.row(), {k: round(r, 3) for k, r in v.ratios().items()})
    assert v.ok != rejected, v.row()


def test_precision_context_restores_the_mode():
    assert not O._Prec.half
    with O.precision("fp16"):
        assert O._Prec.half
        with O.precision("fp32"):
            assert not O._Prec.half
        assert O._Prec.half
    assert not O._Prec.half
    with pytest.raises(ValueError):
        with O.precision("bf16"):
            pass
