"""K1 (s2m2_cost_volume, csrc/ln_corr.hip) through the C ABI against a float64 reference, in the block shapes the forward launches it in.

The planner (csrc/ln_corr_select.h) splits image rows into strips until the grid covers the chip, so a volume of a few rows -- every K1
case of tests/test_hip_dispinit.py -- runs on blocks of one or two waves.  The cases here (tests/k1_cases.py) have 200 rows or blocks that
are full anyway: 3 to 12 waves per block, 1 to 10 chunks of right tokens, waves past the row end that still load tokens and sit in every
barrier, the widest block of every configuration, grids that are no multiple of 8.  tests/test_k1_cases_cpu.py asks the planner for every
claimed plan, and shows that the comparator used here rejects seven wrong variants of the kernel's arithmetic.

Every case: all 15 (token dtype, volume dtype, C), LayerNorm inside the kernel and tokens normalised already; a dense NaN-filled ``out``
(plain stores) and a NaN-filled row-padded view (write-through stores), whose padding must still be NaN afterwards.  Every element is
compared with the float64 reference, evaluated on the device, under the elementwise bounds of k1_cases.py.  Banded launches: the float64
bound and bit-identity with the full launch inside the band, the NaN prefill intact beyond the kernel's own granule limit (k1_cases.band_masks:
with an odd number of tiles per chunk the last pair of a chunk reaches 32 columns into the next one, where a banded launch that skips that
chunk leaves a copy of the previous tile -- beyond the band, inside the limit; the full launch overwrites it and is checked on every element).  The timed
launch (two events on the dispatch: what the benchmark reads K1's time from) writes what the plain one writes.  Ten launches are
bit-identical; exchanging the images transposes the volume bit-exactly on an 11-wave block.
S2M2_K1_BLOCKS_TABLE=<path> writes one line per case: plan, worst error, its bound, their ratio (profiles/k1/k1_blocks.txt)."""
import math
import os

import pytest
import torch

import k1_cases as K

pytestmark = pytest.mark.gpu
TABLE = []
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    path = os.environ.get("S2M2_K1_BLOCKS_TABLE")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(TABLE) + "\n")


def launch(hip, case, inp, **kw):
    cdt = K.TDT[case.cdt]
    if case.form == "ln":
        return hip.ln_corr(inp.tokens, inp.gamma, inp.beta, cv_dtype=cdt, **kw)
    return hip.corr(inp.tokens, cv_dtype=cdt, **kw)


def nan_dense(case):
    B, h, w = case.dims
    return torch.full((B, h, w, w), float("nan"), device=DEV, dtype=K.TDT[case.cdt])


def nan_padded(hip, case):
    """a cv_alloc view whose every element, padding included, is NaN"""
    B, h, w = case.dims
    view = hip.cv_alloc(B, h, w, K.TDT[case.cdt], DEV)
    base = view._base if view._base is not None else view
    base.fill_(float("nan"))
    return view, base


@pytest.mark.parametrize("case", K.all_cases(), ids=lambda c: c.id)
def test_block_shapes_vs_float64(hip, case):
    B, h, w = case.dims
    inp = K.inputs(case.shape, case.tdt, case.C, DEV)
    ref = K.reference(case, DEV)
    dense = nan_dense(case)
    launch(hip, case, inp, out=dense)
    view, base = nan_padded(hip, case)
    launch(hip, case, inp, out=view)
    torch.cuda.synchronize()
    rd, rv = K.compare(dense, ref), K.compare(view, ref)
    TABLE.append(K.line(case, max(rd, rv, key=lambda r: r.ratio), f"  (dense {rd.ratio:.3f}, row-padded {rv.ratio:.3f})"))
    print(TABLE[-1])
    assert rd.ratio <= 1, f"dense out, element {rd.where}: {K.line(case, rd)}"
    assert rv.ratio <= 1, f"row-padded out, element {rv.where}: {K.line(case, rv)}"
    assert base.shape[-1] % (128 // K.BYTES[case.cdt]) == 0
    assert bool(torch.isnan(base[..., w:]).all()), "the padding of a row-padded volume was written"
    assert torch.equal(dense, view), "plain and write-through stores differ"


BAND_CASES = K.cases(shapes="AC", pairs=[("float16", "float16"), ("float32", "float32")], Cs=[128, 256])


@pytest.mark.parametrize("case", BAND_CASES, ids=lambda c: c.id)
def test_banded_launches_vs_float64(hip, case):
    B, h, w = case.dims
    inp = K.inputs(case.shape, case.tdt, case.C, DEV)
    ref = K.reference(case, DEV)
    full = nan_dense(case)
    launch(hip, case, inp, out=full)
    for band in (0, 11, 75, w + 5):
        out = nan_dense(case)
        launch(hip, case, inp, out=out, band=band)
        torch.cuda.synchronize()
        inside, beyond = K.band_masks(case, band, DEV)
        res = K.compare(out, ref, where=inside.expand(B, h, w, w))
        TABLE.append(K.line(case, res, f"  band {band}"))
        print(TABLE[-1])
        assert res.ratio <= 1, f"band {band}, element {res.where}: {K.line(case, res)}"
        assert torch.equal(out[:, :, inside], full[:, :, inside]), f"band {band}: not the full launch's values inside the band"
        assert bool(torch.isnan(out[:, :, beyond]).all()), f"band {band}: written at or beyond the granule limit"
        if band >= w:
            assert not bool(beyond.any()) and torch.equal(out, full)
        elif band <= 11:
            assert bool(beyond.any())


@pytest.mark.parametrize("case", K.cases(shapes="A", Cs=[128]), ids=lambda c: c.id)
def test_timed_launch_writes_what_the_plain_one_writes(hip, case):
    inp = K.inputs(case.shape, case.tdt, case.C, DEV)
    plain, _ = nan_padded(hip, case)
    launch(hip, case, inp, out=plain)
    timed, _ = nan_padded(hip, case)
    timer = hip.KernelTimer()
    launch(hip, case, inp, out=timed, timer=timer)
    torch.cuda.synchronize()
    us = timer.elapsed_us()
    assert math.isfinite(us) and us > 0, us
    assert not bool(torch.isnan(timed).any()) and torch.equal(timed, plain)


def test_ten_launches_are_bit_identical(hip):
    case = K.cases(shapes="A", pairs=[("float16", "float16")], Cs=[128], forms=["pre"])[0]
    inp = K.inputs(case.shape, case.tdt, case.C, DEV)
    first, _ = nan_padded(hip, case)
    launch(hip, case, inp, out=first)
    for _ in range(9):
        again, _ = nan_padded(hip, case)
        launch(hip, case, inp, out=again)
        assert torch.equal(again, first)


def test_swap_is_exact_transpose_on_an_11_wave_block(hip):
    """the property of test_ln_corr_swap_is_exact_transpose (tests/test_hip_dispinit.py) at shape B: fp16, LayerNorm inside, 11 waves"""
    case = K.cases(shapes="B", pairs=[("float16", "float16")], Cs=[128], forms=["ln"])[0]
    assert case.plan.nw == 11 and case.plan.full
    inp = K.inputs(case.shape, case.tdt, case.C, DEV)
    a = launch(hip, case, inp)
    swapped = torch.cat([inp.tokens[inp.B:], inp.tokens[:inp.B]]).contiguous()
    b = hip.ln_corr(swapped, inp.gamma, inp.beta)
    assert torch.equal(a, b.transpose(2, 3))
