"""K3 (s2m2_cv_lookup, csrc/cv_lookup.hip + csrc/cv_lookup.h) against the reference of tests/k3_cases.py -- fp32 coordinates step by step
as the kernel and grid_sample compute them, float64 blend -- on token-like volumes and adversarial disparity rows: integers, exact zeros,
half-integers, x on -1 / 0 / ws - 1 / ws of either level and one ulp to both sides, +-1e-6, +-1e6 and +-1e30, uniform.  Every image row
of a case is one pattern, so a failure names it.  tests/test_k3_cases_cpu.py holds the same reference and comparator against
F.grid_sample, against the fp32 oracle and against seven wrong variants.

  cases     w = 4 (smallest legal), 6 and 10 (odd level-1 width), 8 (narrower than 2r + 1), 72, 128 (w * 2T is exactly 9 blocks), 304 (grid
            tail), 608; radius 0 / 1 / 4 / 16 at w = 8 and 72; B = 2, h = 3 with different content per batch entry; B * h = 65535 (the
            last legal grid row), compared in full
  forms     hip.cv_lookup: volume fp32 / fp16 x output fp32 / fp16 x planar / channels-last, corr1 and corr2 both judged;
            hip.cv_lookup_into (the entry point the engine uses): Cb = 32 at offsets 0 / 16 and Cb = 24 at 3 / 13 (radius 16: 33 taps,
            so Cb = 72 at 0 / 36 and Cb = 80 at 3 / 45), every other channel and a guard pixel behind the buffer keep a sentinel
  bound     k3_cases.bound(): 10 * 2^-24 * max |cv|, plus 2^-11 |ref| + 2^-25 for an fp16 output; derived there, every element judged;
            the taps of the +-1e6 / +-1e30 rows are +0.0 bit for bit.  Observed err / bound: profiles/k3/k3_edges.txt
            (S2M2_K3_EDGES_TABLE=<path> writes the table)
  pitch     the binding takes volume rows a multiple of 8 elements apart, so w = 4, 6, 10 run at pitch 8 with NaN in the padding (the
            C ABI itself takes pitch = w = 4: test_last_grid_row_dense_through_the_abi); row-padded volumes from hip.cv_alloc with NaN
            padding are bit-equal to the dense run on every pattern
  band      K1 with band = 11 into a NaN-filled buffer, then K3 at d >= 0: finite and bit-equal to the lookup on the full volume, and
            what K1 wrote contains the reference's touch set -- which reaches column r + 12 on row r, one past "i + 11"
"""
import os

import pytest
import torch

import k3_cases as K

pytestmark = pytest.mark.gpu
TABLE = []
F16, F32 = torch.float16, torch.float32
SENTINEL = -777.0                         # exact in fp16; no lookup of these volumes returns it
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    from s2m2_amd import hip as h
    h.load()
    return h


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    path = os.environ.get("S2M2_K3_EDGES_TABLE")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(TABLE) + "\n")


def place(cv, dtype, pitch):
    """the CPU volume on the device with rows ``pitch`` elements apart and NaN between them"""
    B, h, w, _ = cv.shape
    full = torch.full((B, h, w, pitch), NAN, device="cuda", dtype=dtype)
    full[..., :w] = cv.to("cuda", dtype)
    return full[..., :w]


def dense(case):
    return place(case.cv, K.TDT[case.dtype], (case.w + 7) // 8 * 8)


def padded(hip, case):
    cv = hip.cv_alloc(case.B, case.h, case.w, K.TDT[case.dtype], "cuda")
    cv.as_strided((case.B, case.h, case.w, cv.stride(2)), cv.stride()).fill_(NAN)
    cv.copy_(case.cv)
    return cv


def judge(case, ref, c1, c2, out_dtype, what, bad):
    res = K.compare(case, ref, c1, c2, out_dtype)
    TABLE.append(K.line(case, what, res))
    print(TABLE[-1])
    bad += [f"{what}: {b}" for b in res.bad]


def into_layouts(radius):
    return ((32, 0, 16), (24, 3, 13)) if radius <= 4 else ((72, 0, 36), (80, 3, 45))


def guarded(case, cb, dtype):
    """(B,h,w,Cb) of sentinels with one more pixel of them behind it"""
    n = case.B * case.h * case.w * cb
    flat = torch.full((n + cb,), SENTINEL, device="cuda", dtype=dtype)
    return flat, flat[:n].view(case.B, case.h, case.w, cb)


def untouched(flat, buf, off1, off2, T):
    cb = buf.shape[-1]
    keep = torch.ones(cb, dtype=torch.bool, device="cuda")
    keep[off1:off1 + T] = False
    keep[off2:off2 + T] = False
    bits = lambda t: t.contiguous().view(torch.int16 if t.dtype == F16 else torch.int32)
    want = bits(torch.tensor([SENTINEL], device="cuda", dtype=buf.dtype))
    return bool((bits(buf[..., keep]) == want).all()) and bool((bits(flat[-cb:]) == want).all())


@pytest.mark.parametrize("dt", ["float32", "float16"], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", K.NAMES)
def test_lookup_vs_reference(hip, name, dt):
    case, ref = K.build(name, dt), K.reference(name, dt)
    cv, disp, T, bad = dense(case), case.disp.cuda(), 2 * case.radius + 1, []
    for out_dtype in (F32, F16):
        for channels_last in (False, True):
            c1, c2 = hip.cv_lookup(cv, disp, case.radius, channels_last, out_dtype)
            assert c1.dtype == c2.dtype == out_dtype
            assert c1.shape == c2.shape == ((case.B, case.h, case.w, T) if channels_last else (case.B, T, case.h, case.w))
            if channels_last:
                c1, c2 = c1.permute(0, 3, 1, 2), c2.permute(0, 3, 1, 2)
            judge(case, ref, c1, c2, out_dtype, f"out {K.SHORT[out_dtype]} {'channels-last' if channels_last else 'planar'}", bad)
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("dt", ["float32", "float16"], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", K.NAMES)
def test_lookup_into_vs_reference(hip, name, dt):
    """B2_h3_w72_r4 is the case that needs batch_stride and pix_stride to be right"""
    case, ref = K.build(name, dt), K.reference(name, dt)
    cv, disp, T, bad = dense(case), case.disp.cuda(), 2 * case.radius + 1, []
    for buf_dtype in (F16, F32):
        for cb, off1, off2 in into_layouts(case.radius):
            flat, buf = guarded(case, cb, buf_dtype)
            hip.cv_lookup_into(cv, disp, buf, off1, off2, case.radius)
            torch.cuda.synchronize()
            what = f"into {K.SHORT[buf_dtype]} Cb {cb} at {off1} / {off2}"
            judge(case, ref, buf[..., off1:off1 + T].permute(0, 3, 1, 2), buf[..., off2:off2 + T].permute(0, 3, 1, 2), buf_dtype, what, bad)
            if not untouched(flat, buf, off1, off2, T):
                bad.append(f"{what}: a channel outside the two tap ranges, or the pixel behind the buffer, lost its sentinel")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("dt", ["float32", "float16"], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", ["w6_r4", "w10_r4", "w8_r16", "w72_r4", "w304_r4", "B2_h3_w72_r4"])
def test_row_padded_volume_is_bit_equal_on_the_adversarial_patterns(hip, name, dt):
    """x0 + 1 on ws, x0 on -1: the taps next to the padding, which continuous random disparities never produce.  NaN times any weight is NaN."""
    case = K.build(name, dt)
    a, b, disp = dense(case), padded(hip, case), case.disp.cuda()
    assert b.stride(2) > a.stride(2) and bool(torch.isnan(b.as_strided((case.B, case.h, case.w, b.stride(2)), b.stride())[..., case.w:]).all())
    for x, y in zip(hip.cv_lookup(a, disp, case.radius), hip.cv_lookup(b, disp, case.radius)):
        assert bool(torch.isfinite(y).all()) and torch.equal(x, y)
    cb, off1, off2 = into_layouts(case.radius)[0]
    bufs = []
    for cv in (a, b):
        bufs.append(torch.full((case.B, case.h, case.w, cb), SENTINEL, device="cuda", dtype=F16))
        hip.cv_lookup_into(cv, disp, bufs[-1], off1, off2, case.radius)
    assert bool(torch.isfinite(bufs[1]).all()) and torch.equal(bufs[0], bufs[1])


def test_last_grid_row_dense_through_the_abi(hip):
    """B * h = 65535 at pitch = w = 4 (4 MB in fp32), which only the C ABI takes: every element against the reference"""
    name = "B255_h257_w4_r4"
    lib, bad = hip.load(), []
    for dt in ("float32", "float16"):
        case, ref = K.build(name, dt), K.reference(name, dt)
        cv, disp = case.cv.to("cuda", K.TDT[dt]), case.disp.cuda()
        B, h, w, T = case.B, case.h, case.w, 2 * case.radius + 1
        out = torch.full((2, B, T, h, w), SENTINEL, device="cuda")
        rc = lib.s2m2_cv_lookup(cv.data_ptr(), disp.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), B, h, w, case.radius, hip._DT[cv.dtype],
                                hip._DT[F32], T * h * w, 1, h * w, w, hip._stream())
        assert rc == 0, lib.s2m2_last_error()
        torch.cuda.synchronize()
        judge(case, ref, out[0], out[1], F32, "C ABI, pitch = w, out fp32 planar", bad)
    assert not bad, "; ".join(bad)


# ---- K1 band -> K3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, F32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("w", [72, 304, 608])
def test_banded_volume_holds_everything_the_lookups_read(hip, w, dtype):
    """S2M2_CV_BAND=1: K1 writes columns j <= i + 11 of each wave's 32 rows, rounded up to its 64-column store granule, and K3 reads the
    rest of the buffer as it finds it.  The lookups of d >= 0 read j <= r + 12 on row r (tests/test_k3_cases_cpu.py): the one column past
    the band is read on rows r % 32 == 31 too (304: row 31), and is inside the granule that holds r + 11."""
    C, h, rad = 128, len(K.BAND_PATTERNS), 4
    g = torch.Generator().manual_seed(1000 + w)
    feat = (torch.randn(2, h, w, C, generator=g) * 1.3 + 0.1).to("cuda", dtype)
    gam = (1 + 0.1 * torch.randn(C, generator=g)).cuda()
    bet = (0.05 * torch.randn(C, generator=g)).cuda()
    disp_cpu = K.disparities((K.BAND_PATTERNS,), w, g)
    assert float(disp_cpu.min()) >= 0
    disp = disp_cpu.cuda()
    full = hip.ln_corr(feat, gam, bet)
    band = torch.full((1, h, w, w), NAN, device="cuda", dtype=dtype)
    hip.ln_corr(feat, gam, bet, out=band, band=11)
    torch.cuda.synchronize()
    assert full.dtype == dtype and bool(torch.isnan(band).any()), "the band left nothing unwritten: this test would show nothing"
    for a, b in zip(hip.cv_lookup(full, disp, rad), hip.cv_lookup(band, disp, rad)):
        assert bool(torch.isfinite(b).all()), "a lookup at d >= 0 read an element the banded K1 never wrote"
        assert torch.equal(a, b)
    ba, bb = (torch.zeros(1, h, w, 32, device="cuda", dtype=dtype) for _ in range(2))
    hip.cv_lookup_into(full, disp, ba, 0, 16, rad)
    hip.cv_lookup_into(band, disp, bb, 0, 16, rad)
    assert bool(torch.isfinite(bb).all()) and torch.equal(ba, bb)
    # the same with a sentinel: what K1 wrote contains every element the reference says the lookups dereference
    marked = torch.full((1, h, w, w), SENTINEL, device="cuda", dtype=dtype)
    hip.ln_corr(feat, gam, bet, out=marked, band=11)
    torch.cuda.synchronize()
    written = (marked != SENTINEL).cpu()
    touch = torch.from_numpy(K.touch_set(disp_cpu, w, rad))
    missing = touch & ~written
    assert not bool(missing.any()), f"{int(missing.sum())} touched elements unwritten, first (b, y, r, j) = {missing.nonzero()[0].tolist()}"
    r = torch.arange(w)[:, None]
    j = torch.arange(w)[None, :]
    assert not bool((touch & (j > r + 12)).any())
    if w == 304:
        assert bool(touch[0, :, 31, 43].any()), "row 31 is no longer read at column 31 + 12"


# ---- refusals: an error from the entry point, nothing launched ---------------------------------------------------------------------------
REFUSED = {                               # B, h, w, radius, cv dtype id, out dtype id, cv_pitch, message
    "odd w": (1, 2, 7, 4, 0, 0, 0, b"must be even"),
    "w = 2": (1, 2, 2, 4, 0, 0, 0, b"at least 4"),
    "w = 0": (1, 2, 0, 4, 0, 0, 0, b"bad arguments"),
    "radius 17": (1, 2, 8, 17, 0, 0, 0, b"bad arguments"),
    "radius -1": (1, 2, 8, -1, 0, 0, 0, b"bad arguments"),
    "B * h = 65536": (256, 256, 4, 4, 0, 0, 0, b"65535"),
    "cv_pitch < w": (1, 2, 8, 4, 0, 0, 4, b"cv_pitch=4"),
    "cv dtype id 2": (1, 2, 8, 4, 2, 0, 0, b"unsupported dtypes cv=2"),
    "out dtype id 7": (1, 2, 8, 4, 1, 7, 0, b"out=7"),
    "cv dtype id -1": (1, 2, 8, 4, -1, 1, 0, b"unsupported dtypes"),
}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_refusals(hip, why):
    B, h, w, radius, cvdt, outdt, pitch, msg = REFUSED[why]
    lib = hip.load()
    T = 2 * abs(radius) + 1
    cv = torch.zeros(B, h, max(w, 1), max(w, pitch, 1), device="cuda")                    # large enough for what the call claims
    disp = torch.zeros(B, 1, h, max(w, 1), device="cuda")
    out = torch.full((2, B, T, h, max(w, 1)), SENTINEL, device="cuda")
    rc = lib.s2m2_cv_lookup(cv.data_ptr(), disp.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), B, h, w, radius, cvdt, outdt,
                            T * h * w, 1, h * w, pitch, hip._stream())
    err = lib.s2m2_last_error()
    torch.cuda.synchronize()
    assert rc != 0 and msg in err, (rc, err)
    assert bool((out == SENTINEL).all()), "a refused call wrote to its outputs"


def test_the_binding_refuses_what_the_kernel_would_misread(hip):
    """on device tensors (tests/test_hip_binding_cpu.py has the helper's cases): an fp16 disp used to be read through a float pointer, and
    an offset past Cb - (2r + 1) used to write into the next pixel"""
    case = K.build("w8_r4")
    cv, disp = dense(case), case.disp.cuda()
    buf = torch.full((1, case.h, 8, 32), SENTINEL, device="cuda", dtype=F16)
    for call in (lambda: hip.cv_lookup_into(cv, disp.half(), buf, 0, 16), lambda: hip.cv_lookup_into(cv, disp, buf, 0, 24),
                 lambda: hip.cv_lookup_into(cv, disp, buf, 4, 12), lambda: hip.cv_lookup_into(cv, disp[..., :4].contiguous(), buf, 0, 16),
                 lambda: hip.cv_lookup_into(cv, disp, buf[:, :3].contiguous(), 0, 16), lambda: hip.cv_lookup(cv, disp.half()),
                 lambda: hip.cv_lookup(cv, disp, 17)):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
