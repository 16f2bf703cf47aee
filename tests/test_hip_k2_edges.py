"""K2 (s2m2_sinkhorn_regress, csrc/sinkhorn.hip) through the C ABI against a float64 reference, at every boundary of its dispatch, on token-like
volumes (tests/k2_cases.py: a match scores 124, a non-match N(0, 11), 5 % of the pixels occluded -- a column spans 150 to 190, five times
the seeded volumes of tests/test_hip_dispinit.py, so the lazy column stabilisers of the exact sweep have to move after the first row, and the dustbin takes whole rows).

Dispatch classes (dispatch_ppl / launch_sinkhorn / K2Lds; tests/test_k2_cases_cpu.py recomputes the limits) and the widths here that reach
them.  TRI (the masked triangle resident in LDS) needs positivity, 16 lanes per row and 160 KB; "plain" is every launch without it.

  lanes x chunks  widths of the class   form, dtype          widths run here
  16 x 1          8 ... 128             TRI   fp16, fp32     8, 16, 128                   (8, 16: fewer columns than a group has lanes;
                                        plain fp16, fp32     8, 16, 128 without positivity;  8: the 5-tap window is wider than the row)
                                                             16 under positivity in the S2M2_K2_TRI=0 child
  16 x 2          136 ... 256           TRI   fp16, fp32     136, 256                     (136: the last chunk is lane 0's alone; 256: full)
                                        plain fp16, fp32     136, 256 without positivity; 136 under positivity in the child
  16 x 3          264 ... 384           TRI   fp16           264, 272, 304, 360           (360: the last fp16 TRI width; 304: the benchmarked launch)
                                        TRI   fp32           264                          (the only fp32 TRI width with three chunks)
                                        plain fp16         * 368, 384 under positivity; all six without; 304 in the child
                                        plain fp32         * 272, 304, 360, 368, 384 under positivity; all six without; 304 in the child
  32 x 2          392 ... 512           plain fp16, fp32     512                          (full last chunk; 392, 400 in test_hip_dispinit.py)
  32 x 3          520 ... 768           plain fp16, fp32     520                          (lane 0's last chunk; 608, 768 in test_hip_dispinit.py)
  64 x 2          776 ... 1024          plain fp16, fp32     1024                         (776, 800 in test_hip_dispinit.py)
  64 x 3          1032 ... 1536         plain fp16, fp32     1032, 1536                   (the widest row; 1544 is refused)
  * masked decoding in global memory (positivity without the triangle) at one and two chunks exists only behind S2M2_K2_TRI=0.

Every case is a two-row volume (one B = 2, h = 3): the planted matches sit at column 0 (from pixels 0 and 1), on the diagonal at the last
column and on both sides of the edge between chunks 0 and 1.  Asserted (k2_cases.check, the comparator tests/test_k2_cases_cpu.py runs
on the fp32 oracle and on wrong variants): argmax equal on every sure and every planted pixel, at most 5 % of the pixels not sure; conf
and disp where the argmax agrees, occ everywhere, with conf, occ < 5e-5 and disp < 2e-4 + 2e-7 w; 0 <= occ <= 1 + 1e-5; all finite.
Two rules follow from the inputs and not from the kernel, both in k2_cases.py with their reasons: a pixel whose largest probability is
below the fp32 range is not sure, and disp on pixels of conf < 1e-2 is judged against three times the fp32 oracle's own distance from
float64 on the same pixels (measured: profiles/r08/k2_edges.txt; S2M2_K2_EDGES_TABLE=<path> writes the table).
"""
import os
import subprocess
import sys

import pytest
import torch

import k2_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = []
LEG = (16, 136, 304)                      # positivity cases the child repeats with S2M2_K2_TRI=0


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    path = os.environ.get("S2M2_K2_EDGES_TABLE")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(TABLE) + "\n")


def run(hip, w, pos, dt, h=2, B=1, ot_iter=3):
    case = K.build(w, pos, dt, h, B)
    ref = K.reference(w, pos, dt, h, B, ot_iter)
    yard = K.yardstick(w, pos, dt, h, B, ot_iter)
    cv = case.cv.to("cuda", K.TDT[dt])
    disp, conf, occ, am = hip.sinkhorn_regress(cv, pos, ot_iter, want_argmax=True)
    assert disp.shape == conf.shape == occ.shape == (B, 1, h, w) and am.shape == (B, h, w) and am.dtype == torch.int32
    e = K.compare(case, ref, disp, conf, occ, am)
    off = os.environ.get("S2M2_K2_TRI") == "0"
    TABLE.append(K.line(case, ot_iter, e, yard, "  S2M2_K2_TRI=0" if off else "", switch_on=not off))
    print(TABLE[-1])
    bad = K.check(case, e, yard)
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("pos", [True, False], ids=["pos", "neg"])
@pytest.mark.parametrize("dt", ["float32", "float16"], ids=["fp32", "fp16"])
@pytest.mark.parametrize("w", K.WIDTHS)
def test_dispatch_boundaries_vs_float64(hip, w, dt, pos):
    run(hip, w, pos, dt)


def test_two_images_three_rows(hip):
    run(hip, 136, True, "float16", h=3, B=2)


@pytest.mark.parametrize("ot_iter", [1, 2, 5])
@pytest.mark.parametrize("w,pos,dt", [(136, True, "float16"), (304, True, "float16"), (520, False, "float32")])
def test_other_sweep_counts(hip, w, pos, dt, ot_iter):
    """ot_iter = 1: the `last` path straight after pass 0; 2 and 5: the fallback flags rotate through all three slots"""
    run(hip, w, pos, dt, ot_iter=ot_iter)


@pytest.mark.parametrize("dt", ["float32", "float16"], ids=["fp32", "fp16"])
@pytest.mark.parametrize("w", LEG)
def test_switch_leg(hip, w, dt):
    """with the triangle here; test_tri_switch_off_in_a_child repeats these with S2M2_K2_TRI=0 (masked decoding from global memory)"""
    run(hip, w, True, dt)


def test_tri_switch_off_in_a_child():
    """read once per process by the library (static const): the positivity cases at 16, 136 and 304 in a fresh child process"""
    env = dict(os.environ, S2M2_K2_TRI="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider", "-s",
                        "-k", "test_switch_leg"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"{2 * len(LEG)} passed" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]


# ---- refusals: an error from the entry point, nothing launched ---------------------------------------------------------------------------
@pytest.mark.parametrize("w,pitch,msg", [(1544, 1544, "too large (max 1536)"), (12, 16, "multiple of 8"), (1532, 1536, "multiple of 8")])
def test_refused_widths(hip, w, pitch, msg):
    cv = torch.zeros(1, 2, w, pitch, device="cuda")[..., :w]
    with pytest.raises(RuntimeError, match=msg.replace("(", r"\(").replace(")", r"\)")):
        hip.sinkhorn_regress(cv, True, 3)
    out = torch.full((4, 1, 1, 2, w), -777.0, device="cuda")
    lib = hip.load()
    for dtype in (torch.float32, torch.float16):
        c = cv.to(dtype) if dtype == torch.float32 else torch.zeros(1, 2, w, pitch, device="cuda", dtype=dtype)[..., :w]
        rc = lib.s2m2_sinkhorn_regress(c.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), 1, 2, w, 3, 1,
                                       hip._DT[dtype], pitch, None, hip._stream())
        assert rc != 0 and msg.encode() in lib.s2m2_last_error()
    torch.cuda.synchronize()
    assert bool((out == -777.0).all()), "a refused call wrote to its outputs"
