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


# ---- the refinement half (module_parity.o_*): mutations the engine's packing of these modules could plausibly have -----------------------
# S weights at w = 304, 16 rows (8 for the full-resolution heads); the disparity regime is the near one unless the name says otherwise.
RH, RW = 16, 304


def _conv_edit(edit):
    """O._conv with (prefix, input) edited: edit(p, x) -> (p, x)"""
    real = O._conv

    def conv(sd, p, x, stride=1, pad=0):
        p, x = edit(p, x)
        return real(sd, p, x, stride, pad)
    return lambda: MP.patched(O, "_conv", conv)


def _lookup_edit(edit):
    real = O.cv_lookup
    return lambda: MP.patched(O, "cv_lookup", lambda cv, disp, radius=4: edit(*real(cv, disp, radius)))


def _swap(a, b):
    def edit(p, x):
        return (p.replace(a, b) if a in p else p.replace(b, a)), x
    return edit


def _blend_exchanged():
    def conv_gru(sd, p, h, x):                                          # O.conv_gru with z and 1 - z exchanged in the blend
        for sfx, pad in (("1", (1, 0)), ("2", (0, 1))):
            hx = torch.cat([h, x], 1)
            z = O._q(torch.sigmoid(O._conv(sd, f"{p}.convz{sfx}", hx, 1, pad)))
            r = O._q(torch.sigmoid(O._conv(sd, f"{p}.convr{sfx}", hx, 1, pad)))
            q = O._q(torch.tanh(O._conv(sd, f"{p}.convq{sfx}", torch.cat([O._q(r * h), x], 1), 1, pad)))
            h = O._q(O._q(z * h) + O._q(O._q(1 - z) * q))
        return h
    return MP.patched(O, "conv_gru", conv_gru)


def _shuffle_transposed(layer):
    real = O._convT

    def convT(sd, p, x, stride=1, pad=0):
        if p.endswith(layer):
            sd = dict(sd)
            sd[p + ".weight"] = sd[p + ".weight"].transpose(2, 3).contiguous()       # (dy, dx) of the 2 x 2 pixel shuffle exchanged
        return real(sd, p, x, stride, pad)
    return lambda: MP.patched(O, "_convT", convT)


def _disp_in_rgb_slot():
    real = O.upsample_mask_1x                                           # conv_disp reads the R plane, conv_rgb's first plane the disparity
    return MP.patched(O, "upsample_mask_1x", lambda sd, p, disp, rgb, f2x: real(sd, p, rgb[:, 0:1], torch.cat([disp, rgb[:, 1:]], 1), f2x))


def _neigh_transposed():
    def neigh9(x):
        B, _, h, w = x.shape
        xp = F.pad(x, (1, 1, 1, 1), mode="replicate")
        return torch.cat([xp[:, :, dy:dy + h, dx:dx + w] for dx in range(3) for dy in range(3)], 1)
    return MP.patched(O, "_neigh9", neigh9)


def _neigh_zero_padded():
    def neigh9(x):
        B, _, h, w = x.shape
        xp = F.pad(x, (1, 1, 1, 1))
        return torch.cat([xp[:, :, dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], 1)
    return MP.patched(O, "_neigh9", neigh9)


def _refine(sd, far=False, first=True):
    xs = MP.refine_inputs(sd, 128, RH, RW, far, 100, masked_occ=not first)
    return lambda: MP.o_refine(sd, *xs, first=first, want_side=first), xs


def _mask4(sd):
    xs = [MP.round16(torch.tanh(MP.seeded((1, 128, 8, RW), 70))), MP.seeded((1, sd[MP.MASK4 + ".conv_y.weight"].shape[1], 16, 2 * RW), 71)]
    return lambda: MP.o_mask4x(sd, *xs), xs


def _mask1(sd):
    xs = [MP.uniform16((1, 1, 32, 4 * RW), 80, 0.0, 4.0 * (RW - 1)), MP.uniform16((1, 3, 32, 4 * RW), 81, -1.0, 1.0),
          MP.seeded((1, sd[MP.MASK4 + ".conv_y.weight"].shape[1], 16, 2 * RW), 82)]
    return lambda: MP.o_mask1x(sd, *xs), xs


def _up4(sd):
    xs = [MP.uniform16((1, 1, 8, RW), 90, 0.0, RW - 1.0), MP.uniform16((1, 1, 8, RW), 91, 0.0, 1.0), MP.uniform16((1, 1, 8, RW), 92, 0.0, 1.0),
          MP.seeded((1, 9, 32, 4 * RW), 93)]
    return lambda: MP.o_upsample4x(sd, *xs), xs


REFINE_CASES = {
    # id: (module under test -> (fn, inputs), mutation)
    "lookup_level2_without_the_16th": (_refine, _lookup_edit(lambda c1, c2: (c1, c2 * 16))),
    "corr_feat2_reads_level1_taps": (_refine, _lookup_edit(lambda c1, c2: (c1, c1))),
    "nine_taps_reversed": (_refine, _lookup_edit(lambda c1, c2: (c1.flip(1), c2.flip(1)))),
    "conf_occ_logits_swapped": (_refine, _conv_edit(lambda p, x: (p, x.flip(1) if p.endswith("conf_occ_feat.0") else x))),
    "disp_not_divided_by_100": (_refine, _conv_edit(lambda p, x: (p, x * 1e2 if p.endswith("refiner.disp_feat.0") else x))),
    "gru_z_r_halves_swapped": (_refine, _conv_edit(_swap(".gru.convz", ".gru.convr"))),
    "gru_blend_z_exchanged": (_refine, lambda: _blend_exchanged()),
    "update_heads_exchanged": (_refine, _conv_edit(_swap("refiner.disp_update.0", "refiner.conf_occ_update.0"))),
    "mask4x_pixel_shuffle_transposed": (_mask4, _shuffle_transposed(".conv_x")),
    "mask4x_out_pixel_shuffle_transposed": (_mask4, _shuffle_transposed(".conv_concat.2")),
    "mask1x_ctx_pixel_shuffle_transposed": (_mask1, _shuffle_transposed(".conv_ctx")),
    "mask1x_disparity_in_the_red_slot": (_mask1, lambda: _disp_in_rgb_slot()),
    "upsample_neighbours_transposed": (_up4, lambda: _neigh_transposed()),
    "upsample_zero_padding": (_up4, lambda: _neigh_zero_padded()),
    "upsample_disparity_not_times_4": (_up4, lambda: MP.patched(MP, "UP4_SCALE", 1.0)),
}
_PAIRS = {}


def _judged(sd, build, mutation=None):
    """verdicts per output of the (mutated) module in the emulation against the comparator, occ outputs with their keep-mask"""
    if build not in _PAIRS:
        fn, xs = build(sd)
        _PAIRS[build] = (fn, xs) + tuple(MP.oracle_pair(fn))
    fn, xs, y32, y16e = _PAIRS[build]
    ym = y16e
    if mutation is not None:
        with mutation(), torch.no_grad(), O.precision("fp16"):
            ym = fn()
    keep = MP.occ_keep(xs[2], y32[1], y16e[1]) if build is _refine else None
    out = []
    for k, (m, a, b) in enumerate(zip(ym, y32, y16e)):
        kp = MP.nhwc(keep) if (keep is not None and k in MP.OCC_OUTPUTS) else None
        if kp is not None:
            assert 1.0 - float(kp.float().mean()) <= MP.MAX_MASKED
        out.append(MP.judge(MP.nhwc(m), MP.nhwc(a), MP.nhwc(b), f"[{k}]", keep=kp))
    return out


@pytest.mark.parametrize("build", [_refine, _mask4, _mask1, _up4], ids=["refine", "mask4x", "mask1x", "upsample4x"])
def test_judge_accepts_the_emulation_of_the_refinement_half(sd, build):
    vs = _judged(sd, build)
    assert all(v.ok for v in vs), "\n".join(v.msg for v in vs if not v.ok)


@pytest.mark.parametrize("name", list(REFINE_CASES))
def test_judge_rejects_refinement_mutation(sd, name):
    build, mutation = REFINE_CASES[name]
    vs = _judged(sd, build, mutation)
    print(name, [k for k, v in enumerate(vs) if not v.ok], [{q: round(r, 2) for q, r in v.ratios().items()} for v in vs])
    assert not all(v.ok for v in vs), f"{name} passed the comparator: " + " / ".join(v.row() for v in vs)


def test_keep_mask_only_narrows_the_statistics(sd):
    """judge(keep=): an error confined to the masked elements is not counted, the same error on a kept element is; the default
    (keep=None) is the unmasked comparison"""
    y32 = MP.seeded((1, 4, 8, 1), 5)
    y16e = y32 + 1e-3 * MP.seeded((1, 4, 8, 1), 6)
    keep = torch.ones_like(y32, dtype=torch.bool)
    keep[0, 0, 0, 0] = False
    bad = y16e.clone()
    bad[0, 0, 0, 0] += 1.0
    assert not MP.judge(bad, y32, y16e).ok and MP.judge(bad, y32, y16e, keep=keep).ok
    bad = y16e.clone()
    bad[0, 1, 1, 0] += 1.0
    assert not MP.judge(bad, y32, y16e, keep=keep).ok
    bad[0, 1, 1, 0] = float("nan")
    keep[0, 1, 1, 0] = False
    assert not MP.judge(bad, y32, y16e, keep=keep).ok          # non-finite values are never masked


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
