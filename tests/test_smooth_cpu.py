"""K29 without a GPU: the numpy oracle of tests/smooth_oracle.py is checked against a scalar, per-pixel transcription of the header's text; the
cases of tests/smooth_cases.py hold what they are meant to hold; the exactly decidable properties of the rule hold; the step of the noisy edge
scene does not bleed; the filter does what it is for (normals and disparities of a noisy map get closer to the clean map's); and ten wrong
kernels are each rejected by some case."""
import numpy as np
import pytest

import cloud_oracle
import normals_oracle as N
import smooth_cases as C
import smooth_oracle as O

F = np.float32
NAMES = [c["name"] for c in C.cases()]
SCALAR_TAPS = 150_000                                        # a case with more pixels x taps than this is transcribed on a sample of its pixels


def _bytes(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.fixture(scope="module")
def oracle():
    return {c["name"]: C.oracle(c, O.tables) for c in C.cases()}


def _scalar(disp, occ, conf, pixels, *, H, W, radius, max_jump, ws, wr, inv, **cam):
    """the header's rule for the pixels (v, u) of `pixels`, one at a time with float32 scalars (one rounding per operation); keep is K15's,
    from cloud_oracle -> {(v, u): (disp_out, taps)}"""
    Hp, Wp = disp.shape
    oy, ox = (Hp - H) // 2, (Wp - W) // 2
    d = np.asarray(disp, F)[oy:oy + H, ox:ox + W]
    keep = cloud_oracle.cloud(d, occ[oy:oy + H, ox:ox + W], conf[oy:oy + H, ox:ox + W], np.zeros((3, H, W), np.uint8), **cam)["keep"]
    gate, inv, top = F(max_jump), F(inv), F(256)
    out = {}
    with np.errstate(all="ignore"):
        for v, u in pixels:
            if not keep[v, u]:
                out[v, u] = (F(-1), 0)
                continue
            num, den, n, dc = F(0), F(0), 0, d[v, u]
            for dv in range(-radius, radius + 1):
                for du in range(-radius, radius + 1):
                    qv, qu = v + dv, u + du
                    if not (0 <= qv < H and 0 <= qu < W) or not keep[qv, qu]:
                        continue
                    e = d[qv, qu] - dc
                    a = abs(e)
                    if not a <= gate:                        # a NaN fails
                        continue
                    t = a * inv
                    t = top if not t < top else t            # fminf(t, 256): the number when t is a NaN
                    i = int(t)
                    w = (ws[abs(dv)] * ws[abs(du)]) * wr[i]
                    num = num + w * e
                    den = den + w
                    n += 1
            assert type(num) is F and type(den) is F
            out[v, u] = (dc + num / den, n)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_the_oracle_is_the_header_text_and_the_case_holds_its_classes(oracle, name):
    c = C.by_name(name)
    o = oracle[name]
    hist = np.bincount(o["cls"].ravel(), minlength=4)
    print(f"[smooth] {name}: " + ", ".join(f"{O.CLASS_NAMES[k]} {hist[k]}" for k in range(4)))
    for k in c["classes"]:
        assert hist[k] > 0, f"{name} was meant to hold pixels of the class '{O.CLASS_NAMES[k]}'"
    H, W, r = c["kw"]["H"], c["kw"]["W"], c["kw"]["radius"]
    ws, wr, inv = O.tables(r, *c["sigma"])
    pixels = [(v, u) for v in range(H) for u in range(W)]
    if len(pixels) * (2 * r + 1) ** 2 > SCALAR_TAPS:         # the corners, and a sample that depends on nothing but the case's size
        pick = np.random.default_rng(H * W + r).choice(len(pixels), SCALAR_TAPS // (2 * r + 1) ** 2, replace=False)
        pixels = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)] + [pixels[i] for i in pick]
    Hp, Wp = c["maps"][0].shape[1:]
    oy, ox = (Hp - H) // 2, (Wp - W) // 2
    for b in range(len(c["maps"][0])):
        s = _scalar(*[m[b] for m in c["maps"]], pixels, **c["kw"], ws=ws, wr=wr, inv=inv)
        for (v, u), (val, n) in s.items():
            got = o["disp_out"][b, 0, oy + v, ox + u]
            assert _bytes(F(val)) == _bytes(got) and n == o["taps"][b, 0, v, u], (name, b, v, u, val, got, n, o["taps"][b, 0, v, u])
        # outside the crop: -1; not kept: -1 and no taps; the count
        border = np.ones((Hp, Wp), bool)
        border[oy:oy + H, ox:ox + W] = False
        assert (o["disp_out"][b, 0][border] == -1).all()
        kept = o["cls"][b] != O.NOT_KEPT
        assert o["count"][b] == kept.sum() and (o["taps"][b, 0][~kept] == 0).all() and (o["taps"][b, 0][kept] >= 1).all()
        assert (o["disp_out"][b, 0, oy:oy + H, ox:ox + W][~kept] == -1).all()


def test_every_class_radius_and_path_is_exercised():
    assert set(k for c in C.cases() for k in c["classes"]) == set(range(4))
    assert {c["kw"]["radius"] for c in C.cases()} >= set(C.RADII)
    assert any(c["kw"]["max_jump"] == float("inf") for c in C.cases()) and any(c["kw"]["max_jump"] == 0.0 for c in C.cases())
    assert any(c["kw"].get("filtered") is False for c in C.cases()) and any(len(c["maps"][0]) == 2 for c in C.cases())
    assert any(c["maps"][0].shape[2] % 4 for c in C.cases()) and any(((c["maps"][0].shape[2] - c["kw"]["W"]) // 2) % 4 for c in C.cases())


def test_the_tables():
    for r, ss, sr in ((1, 0.5, 0.03), (8, 4.0, 0.06), (3, 2.0, 1e-3), (5, 100.0, 50.0)):
        ws, wr, inv = O.tables(r, ss, sr)
        assert ws.dtype == F and wr.dtype == F and type(inv) is F and ws[0] == 1 and wr[0] == 1
        assert (np.diff(ws[:r + 1]) <= 0).all() and not ws[r + 1:].any() and (np.diff(wr) <= 0).all()
        assert abs(float(wr[256]) - np.exp(-8.0)) < 1e-9 and inv == F(64.0 / sr)


# ---- the exactly decidable properties

def _run(disp, kw, *, radius, sigma_r, max_jump, sigma_s=None, **wrong):
    ws, wr, inv = O.tables(radius, radius / 2.0 if sigma_s is None else sigma_s, sigma_r)
    ones = np.ones_like(disp)
    return O.smooth(disp, ones, ones, **kw, radius=radius, max_jump=max_jump, ws=ws, wr=wr, inv=inv, **wrong)


def test_a_constant_map_is_a_fixed_point_at_radius_8():
    kw = dict(C.NC.CAM, H=21, W=30, cx=15.0, cy=10.0)
    disp = np.full((27, 36), 0.7, F)
    o = _run(disp, kw, radius=8, sigma_r=0.03, max_jump=0.25)
    assert (o["disp_out"][3:24, 3:33] == F(0.7)).all() and o["count"] == 21 * 30 and o["taps"].max() == 289 and o["taps"].min() == 81


def test_a_zero_gate_returns_the_input_and_a_lonely_pixel_is_unchanged():
    c = C.by_name("steps_gate0")
    o = C.oracle(c, O.tables)
    d = c["maps"][0][0]
    assert (o["cls"] == O.ALONE).all() and (o["taps"] == 1).all()
    assert _bytes(o["disp_out"][0, 0, 3:27, 4:44]) == _bytes(d[3:27, 4:44])
    # one pixel 5 px above a plane: every neighbour fails the gate, it comes back unchanged; its neighbours lose one tap and nothing else
    kw = dict(C.NC.CAM, H=9, W=9, cx=4.0, cy=4.0)
    disp = np.full((9, 9), 0.5, F)
    disp[4, 4] = 5.5
    o = _run(disp, kw, radius=2, sigma_r=0.03, max_jump=0.25)
    assert o["disp_out"][4, 4] == F(5.5) and o["taps"][4, 4] == 1 and o["cls"][4, 4] == O.ALONE
    assert o["taps"][2, 2] == 24 and o["taps"][0, 0] == 9 and o["cls"][2, 2] == O.GATED and (np.delete(o["disp_out"].ravel(), 40) == F(0.5)).all()


def test_an_open_gate_stays_finite_on_finite_maps():
    for name in ("steps_joined", "own_r8"):
        c = C.by_name(name)
        o = C.oracle(dict(c, kw=dict(c["kw"], max_jump=float("inf"))), O.tables)
        assert np.isfinite(o["disp_out"]).all() and (o["cls"] != O.GATED).all()


def test_two_pairs_are_independent(oracle):
    o = oracle["two_pairs"]
    c = C.by_name("two_pairs")
    for b in range(2):
        one = C.oracle(dict(c, maps=tuple(m[b:b + 1] for m in c["maps"])), O.tables)
        for k in ("disp_out", "taps", "count"):
            assert _bytes(o[k][b]) == _bytes(one[k][0])
    assert _bytes(o["disp_out"][0]) != _bytes(o["disp_out"][1])


# ---- the edge and the purpose

def test_the_step_does_not_bleed_below_the_gate(oracle):
    """columns 0..44 and 45..66 of the result equal each side filtered alone, byte for byte: the smallest difference across the step within
    three columns is above the gate, the largest within a side below it"""
    (disp, occ, conf), kw = C.edge_scene()
    cross = min(np.abs(disp[:, 45 + a] - disp[:, 44 - b]).min() for a in range(3) for b in range(3 - a))
    print(f"[smooth] edge: smallest difference across the step within three columns {cross:.3f} px")
    assert cross > 0.25
    whole = oracle["edge"]["disp_out"][0, 0]
    ws, wr, inv = O.tables(3, 2.0, 0.06)
    rule = dict(radius=3, max_jump=0.25, ws=ws, wr=wr, inv=inv)
    left = O.smooth(disp[:, :45].copy(), occ[:, :45], conf[:, :45], **dict(kw, W=45), **rule)
    right = O.smooth(disp[:, 45:].copy(), occ[:, 45:], conf[:, 45:], **dict(kw, W=22), **rule)
    assert _bytes(whole[:, :45]) == _bytes(left["disp_out"]) and _bytes(whole[:, 45:]) == _bytes(right["disp_out"])
    assert _bytes(oracle["edge"]["taps"][0, 0][:, :45]) == _bytes(left["taps"])
    opened = oracle["edge_open"]["disp_out"][0, 0]
    assert _bytes(opened[:, :45]) != _bytes(left["disp_out"]) and _bytes(opened[:, 45:]) != _bytes(right["disp_out"])


def test_smoothing_halves_the_normal_and_disparity_errors(oracle):
    """the purpose: normals_oracle at radius 1 on the noisy map, on the smoothed map and on the clean map"""
    (clean, occ, conf), kw = C.edge_scene(noise=False)
    (noisy, _, _), _ = C.edge_scene()
    smoothed = oracle["edge_open"]["disp_out"][0, 0]
    rule = dict(radius=1, max_jump=1.0, min_cos=0.0)
    ref = N.normals(clean, occ, conf, **kw, **rule)

    def angle(d, filtered):
        o = N.normals(d, occ, conf, **dict(kw, filtered=filtered), **rule)
        both = (o["cls"] == N.USED) & (ref["cls"] == N.USED)
        dot = (o["normals"].astype(np.float64) * ref["normals"]).sum(0)[both]
        return np.degrees(np.arccos(np.clip(dot, -1, 1))).mean(), both.sum()

    (a0, n0), (a1, n1) = angle(noisy, True), angle(smoothed, False)
    r0 = np.sqrt(((noisy.astype(np.float64) - clean) ** 2).mean())
    r1 = np.sqrt(((smoothed.astype(np.float64) - clean) ** 2).mean())
    print(f"[smooth] mean angle to the clean normals {a0:.1f} -> {a1:.1f} degrees ({a1 / a0:.3f}, {n0} / {n1} pixels), "
          f"RMS disparity error {r0:.4f} -> {r1:.4f} px ({r1 / r0:.3f})")
    assert n0 > 2500 and n1 > 2500
    assert a1 <= a0 / 2 and r1 <= r0 / 2


# ---- wrong kernels

WRONG = dict(jump_scaled="the jump scaled by the radius", gate_running_mean="the gate taken against the running mean",
             index_rounded="i rounded instead of truncated", no_clamp="no clamp at 256", column_major="the window visited column-major",
             ws_of_sum="ws[|dv| + |du|] instead of the product", no_crop="the crop offset dropped",
             padded_neighbours="padded pixels used as neighbours", mean_of_dq="the weighted mean of d_q instead of d_c + num / den",
             radius_one="radius ignored")


@pytest.mark.parametrize("wrong", list(WRONG))
def test_a_wrong_kernel_is_rejected(oracle, wrong):
    rejected = []
    for c in C.cases():
        good, bad = oracle[c["name"]], C.oracle(c, O.tables, **{wrong: True})
        if any(_bytes(good[k]) != _bytes(bad[k]) for k in ("disp_out", "taps", "count")):
            rejected.append(c["name"])
    print(f"[smooth] {WRONG[wrong]}: rejected by {rejected}")
    assert rejected, f"no case tells the rule from: {WRONG[wrong]}"
