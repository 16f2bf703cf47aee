"""The operand vocabulary of s2m2_amd/hip.py on CPU tensors: the geometry helpers are pure functions of shape, stride and dtype, and every
launching wrapper refuses host tensors before it touches the library."""
import pytest
import torch

from s2m2_amd import hip

F16, F32 = torch.float16, torch.float32


# ------------------------------------------------------------------------------------------------ _rows / _pixels
def test_rows_and_pixels_take_a_channel_slice_and_return_its_stride():
    buf = torch.zeros(2, 3, 4, 16)
    x = buf[..., 4:12]
    assert not x.is_contiguous()
    assert hip._rows(x, "t") == (24, 16) and hip._pixels(x, "t") == 16
    assert hip._rows(buf, "t") == (24, 16) and hip._pixels(buf, "t") == 16
    assert hip._rows(torch.zeros(5, 8), "t") == (5, 8) and hip._rows(torch.zeros(8), "t") == (1, 8)
    assert hip._rows(torch.zeros(3, 7, 24)[..., 8:16], "t") == (21, 24)


@pytest.mark.parametrize("helper", [hip._rows, hip._pixels])
def test_rows_and_pixels_reject_what_a_single_stride_cannot_describe(helper):
    x = torch.zeros(2, 3, 4, 8)
    with pytest.raises(ValueError):
        helper(x.transpose(2, 3), "t")                                  # channels not contiguous
    with pytest.raises(ValueError):
        helper(x[..., ::2], "t")
    for dim, stride in ((0, 128), (1, 40)):                             # one outer stride perturbed: rows no longer evenly spaced
        st = list(x.stride())
        st[dim] = stride
        with pytest.raises(ValueError):
            helper(torch.zeros(512).as_strided((2, 3, 4, 8), st), "t")
    with pytest.raises(ValueError):
        helper(torch.zeros(2, 6, 4, 8)[:, ::2], "t")                    # every other image row


def test_pixels_wants_four_dimensions():
    with pytest.raises(ValueError):
        hip._pixels(torch.zeros(3, 4, 8), "t")


@pytest.mark.parametrize("helper", [hip._rows, hip._pixels])
def test_size_one_outer_dimensions_may_have_any_stride(helper):
    base = torch.zeros(4096)
    assert helper(base.as_strided((1, 3, 4, 8), (7, 64, 16, 1)), "t") in ((12, 16), 16)
    assert helper(base.as_strided((1, 1, 4, 8), (5, 3, 16, 1)), "t") in ((4, 16), 16)
    inner = base.as_strided((2, 1, 4, 8), (64, 999, 16, 1))             # a size-1 dimension BETWEEN real ones
    assert hip._pixels(inner, "t") == 16
    with pytest.raises(ValueError):                                     # _rows measures each stride against the next dimension's, as it always did
        hip._rows(inner, "t")


def test_cv_pitch_is_pure_geometry():
    assert hip._cv_pitch(torch.zeros(2, 3, 8, 8), "t") == 8
    assert hip._cv_pitch(torch.zeros(2, 3, 8, 64)[..., :8], "t") == 64
    with pytest.raises(ValueError):
        hip._cv_pitch(torch.zeros(2, 3, 8, 12)[..., :8], "t")           # pitch no multiple of 8
    with pytest.raises(ValueError):
        hip._cv_pitch(torch.zeros(2, 3, 8, 7), "t")
    with pytest.raises(ValueError):
        hip._cv_pitch(torch.zeros(2, 6, 8, 8)[:, ::2], "t")


def _lookup_operands(B=2, h=3, w=8, cb=32, buf_dtype=F16):
    return torch.zeros(B, h, w, w, dtype=F16), torch.zeros(B, 1, h, w), torch.zeros(B, h, w, cb, dtype=buf_dtype)


def test_lookup_geometry_accepts_what_the_engine_passes():
    cv, disp, buf = _lookup_operands()
    assert hip._lookup_geometry("t", cv, disp, 4) == 8
    assert hip._lookup_geometry("t", cv, disp, 4, buf, 0, 16) == 8
    assert hip._lookup_geometry("t", torch.zeros(2, 3, 8, 64)[..., :8], disp, 4, buf.float(), 16, 0) == 64
    for r, cb, o1, o2 in ((0, 2, 0, 1), (0, 2, 1, 0), (16, 66, 0, 33), (4, 24, 3, 13), (4, 18, 9, 0), (4, 32, 23, 14)):
        hip._lookup_geometry("t", cv, disp, r, torch.zeros(2, 3, 8, cb), o1, o2)


def test_lookup_geometry_disp_is_the_fp32_map_of_the_volume():
    cv, disp, buf = _lookup_operands()
    for bad in (disp.half(), disp.double(), disp.int(),                  # read through a float pointer whatever it holds
                torch.zeros(2, 3, 8), torch.zeros(2, 1, 3, 9), torch.zeros(2, 1, 4, 8), torch.zeros(1, 1, 3, 8), torch.zeros(2, 2, 3, 8),
                torch.zeros(2, 1, 3, 16)[..., ::2], torch.zeros(2, 1, 8, 3).transpose(2, 3)):
        with pytest.raises(ValueError, match="t: disp must be"):
            hip._lookup_geometry("t", cv, bad, 4)
        with pytest.raises(ValueError, match="t: disp must be"):
            hip._lookup_geometry("t", cv, bad, 4, buf, 0, 16)
    with pytest.raises(ValueError, match="cv must be fp16 or fp32"):
        hip._lookup_geometry("t", cv.double(), disp, 4)
    with pytest.raises(ValueError, match=r"cv must be a \(B,h,w,w\)"):
        hip._lookup_geometry("t", torch.zeros(2, 3, 8, 10), disp, 4)


@pytest.mark.parametrize("radius", [-1, 17, 4.0, None])
def test_lookup_geometry_radius(radius):
    cv, disp, buf = _lookup_operands(cb=80)
    with pytest.raises(ValueError, match="radius"):
        hip._lookup_geometry("t", cv, disp, radius)
    with pytest.raises(ValueError, match="radius"):
        hip._lookup_geometry("t", cv, disp, radius, buf, 0, 40)


def test_lookup_geometry_buf_and_its_tap_ranges():
    cv, disp, buf = _lookup_operands()
    for bad in (torch.zeros(2, 3, 8, 32, dtype=torch.float64), torch.zeros(2, 3, 8, 32, dtype=torch.bfloat16), torch.zeros(2, 3, 9, 32),
                torch.zeros(2, 4, 8, 32), torch.zeros(1, 3, 8, 32), torch.zeros(2 * 3 * 8, 32), torch.zeros(2, 3, 8, 64)[..., :32],
                torch.zeros(2, 3, 8, 64)[..., ::2], torch.zeros(2, 3, 32, 8).transpose(2, 3)):
        with pytest.raises(ValueError, match="t: buf must be"):
            hip._lookup_geometry("t", cv, disp, 4, bad, 0, 16)
    # radius 4: nine channels per level.  An offset past Cb - 9 writes into the next pixel and, at the last pixel, past the buffer
    for o1, o2 in ((-1, 16), (0, -9), (24, 0), (0, 24), (32, 0), (0, 1 << 40), (0.0, 16), (None, 16)):
        with pytest.raises(ValueError, match="must lie inside the 32 channels"):
            hip._lookup_geometry("t", cv, disp, 4, buf, o1, o2)
    for o1, o2 in ((0, 0), (0, 8), (8, 0), (10, 2), (23, 15)):
        with pytest.raises(ValueError, match="overlap"):
            hip._lookup_geometry("t", cv, disp, 4, buf, o1, o2)
    with pytest.raises(ValueError, match="must lie inside the 8 channels"):
        hip._lookup_geometry("t", cv, disp, 4, torch.zeros(2, 3, 8, 8), 0, 0)
    with pytest.raises(ValueError, match="must lie inside the 32 channels"):
        hip._lookup_geometry("t", cv, disp, 16, buf, 0, 16)               # 33 taps do not fit 32 channels


def test_lookup_wrappers_refuse_bad_operands_before_the_library(monkeypatch):
    """both wrappers go through the helper: on operands that pass the residency check the refusal comes before any library call"""
    monkeypatch.setattr(hip, "_lib", _NoLibrary())
    monkeypatch.setattr(hip, "_resident", lambda what, *ts: None)
    cv, disp, buf = _lookup_operands()
    with pytest.raises(ValueError, match="cv_lookup: disp must be"):
        hip.cv_lookup(cv, disp.half())
    with pytest.raises(ValueError, match="cv_lookup: radius"):
        hip.cv_lookup(cv, disp, 17)
    with pytest.raises(ValueError, match="out_dtype"):
        hip.cv_lookup(cv, disp, 4, False, torch.bfloat16)
    with pytest.raises(ValueError, match="cv_lookup_into: disp must be"):
        hip.cv_lookup_into(cv, disp.half(), buf, 0, 16)
    with pytest.raises(ValueError, match="cv_lookup_into: off2=24"):
        hip.cv_lookup_into(cv, disp, buf, 0, 24)
    with pytest.raises(ValueError, match="cv_lookup_into: .*overlap"):
        hip.cv_lookup_into(cv, disp, buf, 0, 8)
    with pytest.raises(ValueError, match="cv_lookup_into: buf must be"):
        hip.cv_lookup_into(cv, disp, buf[:, :2], 0, 16)


# ------------------------------------------------------------------------------------------------ _vec / _mat / _frag
def test_vec_exact_and_at_least():
    v = torch.zeros(16)
    hip._vec(v, 16, "t")
    hip._vec(v.view(1, 16), 16, "t")
    hip._vec(v, 12, "t", at_least=True)
    hip._vec(v, 16, "t", at_least=True)
    hip._vec(None, 16, "t", optional=True)
    hip._vec(torch.zeros(16, dtype=torch.int32), 16, "t", dtype=torch.int32)
    for bad in (dict(n=12), dict(n=17), dict(n=17, at_least=True)):
        n = bad.pop("n")
        with pytest.raises(ValueError, match="t must be"):
            hip._vec(v, n, "t", **bad)
    with pytest.raises(ValueError):
        hip._vec(v.half(), 16, "t")                                     # wrong dtype
    with pytest.raises(ValueError):
        hip._vec(v, 16, "t", dtype=F16)
    with pytest.raises(ValueError):
        hip._vec(torch.zeros(32)[::2], 16, "t")                         # right count, every other element
    with pytest.raises(ValueError):
        hip._vec(torch.zeros(32)[::2], 8, "t", at_least=True)
    with pytest.raises(ValueError, match="t is missing"):
        hip._vec(None, 16, "t")                                         # a required operand is not optional


def test_mat_off_by_one_in_each_dimension():
    m = torch.zeros(6, 8, dtype=F16)
    hip._mat(m, (6, 8), F16, "t")
    for shape in ((5, 8), (7, 8), (6, 7), (6, 9), (6, 8, 1), (48,)):
        with pytest.raises(ValueError):
            hip._mat(m, shape, F16, "t")
    with pytest.raises(ValueError):
        hip._mat(m, (6, 8), F32, "t")
    with pytest.raises(ValueError):
        hip._mat(torch.zeros(6, 16, dtype=F16)[:, :8], (6, 8), F16, "t")


def test_frag_off_by_one_in_each_dimension():
    cout, k = 40, 72                                                    # -> (2, 5, 64, 8)
    hip._frag(torch.zeros(2, 5, 64, 8, dtype=F16), cout, k, F16, "t")
    for shape in ((1, 5, 64, 8), (3, 5, 64, 8), (2, 4, 64, 8), (2, 6, 64, 8), (2, 5, 63, 8), (2, 5, 65, 8), (2, 5, 64, 7), (2, 5, 64, 9),
                  (2 * 5 * 64 * 8,)):
        with pytest.raises(ValueError, match="pack.x_frag"):
            hip._frag(torch.zeros(shape, dtype=F16), cout, k, F16, "t (pack.x_frag)")
    with pytest.raises(ValueError):
        hip._frag(torch.zeros(2, 5, 64, 8), cout, k, F16, "t")
    with pytest.raises(ValueError):
        hip._frag(torch.zeros(2, 5, 64, 16, dtype=F16)[..., :8], cout, k, F16, "t")
    hip._frag(torch.zeros(1, 1, 64, 8, dtype=F16), 32, 16, F16, "t")     # exact tiles: no rounding up
    with pytest.raises(ValueError):
        hip._frag(torch.zeros(1, 1, 64, 8, dtype=F16), 33, 16, F16, "t")
    with pytest.raises(ValueError):
        hip._frag(torch.zeros(1, 1, 64, 8, dtype=F16), 32, 17, F16, "t")


# ------------------------------------------------------------------------------------------------ residency
def test_resident_names_device_tensors():
    hip._resident("t")
    hip._resident("t", None, None)
    with pytest.raises(ValueError, match="t: .*device tensors"):
        hip._resident("t", None, torch.zeros(1))
    with pytest.raises(ValueError, match="device tensors"):
        hip._resident("t", torch.zeros(1, device="meta"))


class _On:
    """what _resident reads of a tensor, placed on a device this machine need not have"""

    def __init__(self, device):
        self.device, self.is_cuda = torch.device(device), torch.device(device).type == "cuda"


def test_resident_wants_one_device():
    hip._resident("t", _On("cuda:0"))
    hip._resident("t", None, _On("cuda:1"), None, _On("cuda:1"), None)
    for ts in ((_On("cuda:0"), _On("cuda:1")), (_On("cuda:1"), None, _On("cuda:0")), (_On("cuda:0"), _On("cuda:0"), None, _On("cuda:1"))):
        with pytest.raises(ValueError, match="t: .*device tensors on one device, got cuda:. and cuda:."):
            hip._resident("t", *ts)
    with pytest.raises(ValueError, match="device tensors, got one on cpu"):     # a host operand is named as such, whatever came before it
        hip._resident("t", _On("cuda:0"), _On("cpu"))


class _NoLibrary:
    """stands where the loaded library would: any entry point a wrapper reaches for fails the test"""

    def __getattr__(self, name):
        pytest.fail(f"the binding reached the library ({name}) with host operands")


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(hip, "_lib", _NoLibrary())
    assert isinstance(hip.load(), _NoLibrary)


def _wrapper_calls():
    C = 128
    x = torch.zeros(1, 2, 8, C, dtype=F16)                              # (N,H,W,C)
    w = torch.zeros(C, C, dtype=F16)
    b = torch.zeros(C)
    cv = torch.zeros(1, 2, 8, 8, dtype=F16)
    m = torch.zeros(1, 1, 2, 8)                                         # (B,1,h,w) map
    tok = torch.zeros(2, 2, 8, C, dtype=F16)
    frag = torch.zeros(4, 8, 64, 8, dtype=F16)                          # pack.pw_frag of (128, 128)
    img = torch.zeros(1, 3, 32, 32, dtype=torch.uint8)
    rec = torch.zeros(2, hip.RECTIFY_RECORD_FLOATS)
    qkv = torch.zeros(2, 16, 3 * C, dtype=F16)
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    stage = [(w, b, hip.ACT_NONE, None)]
    return {
        "pack_frag": lambda: hip.pack_frag(hip.PACK_ROWS, w),
        "ln_corr": lambda: hip.ln_corr(tok, b, b),
        "corr": lambda: hip.corr(tok),
        "sinkhorn_regress": lambda: hip.sinkhorn_regress(cv, True),
        "cv_lookup": lambda: hip.cv_lookup(cv, m),
        "cv_lookup_into": lambda: hip.cv_lookup_into(cv, m, torch.zeros(1, 2, 8, 32, dtype=F16), 0, 9),
        "conv2d": lambda: hip.conv2d(x, w, b, 1, 1, C),
        "mlp_fan": lambda: hip.mlp_fan(x, w, b, None),
        "mlp_chain": lambda: hip.mlp_chain(x, stage),
        "conv_block": lambda: hip.conv_block(x, torch.zeros(9 * C * C, dtype=F16), b, torch.zeros(9 * C * C, dtype=F16), b, w, b, w, b),
        "row_attn": lambda: hip.row_attn(x, 1, False, torch.zeros(6 * C, C, dtype=F16), torch.zeros(12, C)),
        "pw_direct": lambda: hip.pw_direct([x], frag, b, C),
        "conv_narrow": lambda: hip.conv_narrow(x, torch.zeros(4, 72, 64, 8, dtype=F16), b, 3, 3, C),
        "feature_fusion": lambda: hip.feature_fusion(x, x, torch.zeros(3 * C, 2 * C, dtype=F16), torch.zeros(3 * C), torch.zeros(C, 3 * C, dtype=F16), b, b),
        "layernorm": lambda: hip.layernorm(x),
        "groupnorm_nhwc": lambda: hip.groupnorm_nhwc(x, 8, b, b),
        "convex_upsample": lambda: hip.convex_upsample([m], torch.zeros(1, 8, 32, 16, dtype=F16), 4),
        "attention": lambda: hip.attention(q, k, v, 4),
        "resample2x": lambda: hip.resample2x(x, 0),
        "image_prep": lambda: hip.image_prep(img, img, F16),
        "clock_probe": lambda: hip.clock_probe(torch.zeros(2, dtype=torch.int64)),
        "refine_prep": lambda: hip.refine_prep(m, m, m, 1, F16),
        "global_update": lambda: hip.global_update(torch.zeros(1, 2, 8, 8, dtype=F16), m, m, True),
        "refine_update": lambda: hip.refine_update(torch.zeros(1, 2, 8, 16, dtype=F16), m, m, m, True),
        "tanh": lambda: hip.tanh(x),
        "stem_mlp": lambda: hip.stem_mlp(torch.zeros(1, 2, 8, 8, dtype=F16), torch.zeros(16, 8), torch.zeros(16), torch.zeros(16, 16), torch.zeros(16)),
        "image_pad": lambda: hip.image_pad(img),
        "cloud": lambda: hip.cloud(torch.zeros(1, 1, 32, 32), torch.zeros(1, 1, 32, 32), torch.zeros(1, 1, 32, 32), img, fx=1.0, fy=1.0, cx=0.0, cy=0.0,
                                   baseline=1.0, depth=torch.zeros(1, 1, 32, 32)),
        "rectify": lambda: hip.rectify([torch.zeros(48, 64, 3, dtype=torch.uint8)] * 2, rec, torch.zeros(2, 3, 48, 64)),
    }


WRAPPERS = sorted(_wrapper_calls())


def test_the_table_covers_every_launching_wrapper():
    """every public function of the binding that takes a tensor is in the table above (the *_supported queries, attention_plan, cv_alloc and
    the workspace-size queries take none)"""
    import inspect
    public = {n for n, f in vars(hip).items() if inspect.isfunction(f) and f.__module__ == hip.__name__ and not n.startswith("_")}
    no_tensor = {n for n in public if n.endswith("_supported")} | {"load", "cv_alloc", "cloud_workspace_bytes", "poison_lds", "attention_plan"}
    assert public - no_tensor == set(WRAPPERS)


@pytest.mark.parametrize("name", WRAPPERS)
def test_host_operands_are_refused_before_the_library_is_touched(no_library, name):
    with pytest.raises(ValueError, match="device tensors"):
        _wrapper_calls()[name]()


# The operands whose residency nothing checked before.  With host tensors everywhere the first operand already stops the call, so here
# each is looked for in the wrapper's one residency check; as the ONLY host operand they run on the GPU (tests/test_hip_binding_args.py).
HOLES = {
    "conv2d": ("weight", "bias", "ln_wsum", "bias2"),
    "layernorm": ("x", "out"),
    "mlp_chain": ("res",),
    "feature_fusion": ("z0", "z1"),
    "convex_upsample": ("chan_out",),
}


@pytest.mark.parametrize("name", sorted(HOLES))
def test_the_closed_holes_are_in_the_residency_check(monkeypatch, no_library, name):
    """the wrapper hands every operand that used to go unchecked to _resident, in one call, before anything else can fail"""
    # This looks at how the wrappers are written today (one _resident call, named after the wrapper), which is more than the contract:
    # a wrapper that checked residency in two calls would be as sound.  The behaviour itself -- each of these operands, as the only host
    # tensor of an otherwise valid call, is refused without a library call -- is tests/test_hip_binding_args.py, and that is the test
    # that matters; this one only lets a machine without a GPU notice an operand dropped from the list.
    import inspect
    seen = []

    class Stop(Exception):
        pass

    def spy(what, *ts):
        seen.append((what, ts))
        raise Stop

    monkeypatch.setattr(hip, "_resident", spy)
    C = 128
    x = torch.zeros(1, 2, 8, C, dtype=F16)
    marks = {p: torch.zeros(C) for p in HOLES[name]}
    kw = {
        "conv2d": dict(srcs=x, weight=marks.get("weight"), bias=marks.get("bias"), KH=1, KW=1, Cout=C, ln_wsum=marks.get("ln_wsum"), bias2=marks.get("bias2")),
        "layernorm": dict(x=marks.get("x"), out=marks.get("out")),
        "mlp_chain": dict(x=x, stages=[], res=marks.get("res")),
        "feature_fusion": dict(z0=marks.get("z0"), z1=marks.get("z1"), w1=x, b1=x, w2=x, bg=x, bf=x),
        "convex_upsample": dict(maps=[x], logits=x, factor=4, chan_out=marks.get("chan_out")),
    }[name]
    assert set(HOLES[name]) <= set(inspect.signature(getattr(hip, name)).parameters)
    with pytest.raises(Stop):
        getattr(hip, name)(**kw)
    (what, ts), = seen
    assert what == name
    for p, t in marks.items():
        assert any(t is s for s in ts), f"{name}: {p} is not residency-checked"


def test_plan_pointer_array():
    a = hip._ptrs([None, torch.zeros(4), None])
    assert len(a) == 3 and a[0] is None and a[2] is None and a[1] != 0
    assert len(hip._ptrs([])) == 1                                      # never empty: the C side is handed its address
    assert hip._ptr(None) is None


def test_event_bracket_is_inert_without_a_list():
    with hip._bracket(None, 1.0, "tag"):
        pass
