"""K28 without a GPU: the numpy oracle of tests/normals_oracle.py is checked against a scalar, per-pixel transcription of the header's text; the
cases of tests/normals_cases.py hold what they are meant to hold; the normals point to the side K26's gradients point to; eight wrong kernels
are each rejected by some case; and the normal map of one frame tracks the next through K27's oracle (frame-to-frame odometry)."""
import math

import numpy as np
import pytest

import cloud_oracle
import normals_cases as C
import normals_oracle as N
import tsdf_scenes as S
import tsdf_track_oracle as T
import tsdf_track_scenes as TS

F = np.float32
NAMES = [c["name"] for c in C.cases()]


def _bytes(a):
    return np.ascontiguousarray(a).tobytes()


def _scalar(disp, occ, conf, *, H, W, fx, fy, cx, cy, radius, max_jump, min_cos, **cam):
    """the header's rule, one pixel at a time with float32 scalars (one rounding per operation); keep and z are K15's, from cloud_oracle"""
    Hp, Wp = disp.shape
    oy, ox = (Hp - H) // 2, (Wp - W) // 2
    d = np.asarray(disp, F)[oy:oy + H, ox:ox + W]
    c = cloud_oracle.cloud(d, occ[oy:oy + H, ox:ox + W], conf[oy:oy + H, ox:ox + W], np.zeros((3, H, W), np.uint8), fx=fx, fy=fy, cx=cx, cy=cy, **cam)
    keep, z = c["keep"], c["depth"]
    gate = F(max_jump) * F(radius)
    fx, fy, cx, cy, min_cos = F(fx), F(fy), F(cx), F(cy), F(min_cos)
    nrm, img, cls = np.zeros((3, H, W), F), np.zeros((3, H, W), np.uint8), np.zeros((H, W), np.int8)

    def point(v, u):
        return ((F(u) - cx) * z[v, u] / fx, (F(v) - cy) * z[v, u] / fy, z[v, u])

    def usable(v, u, dc):
        if not (0 <= v < H and 0 <= u < W) or not keep[v, u]:
            return False
        return bool(abs(d[v, u] - dc) <= gate)                 # False for a NaN

    def diff(pc, plus, minus, dc):
        up, um = usable(*plus, dc), usable(*minus, dc)
        a = point(*plus) if up else pc
        b = point(*minus) if um else pc
        return (a[0] - b[0], a[1] - b[1], a[2] - b[2]), up or um

    with np.errstate(all="ignore"):
        for v in range(H):
            for u in range(W):
                if not keep[v, u]:
                    cls[v, u] = N.NOT_KEPT
                    continue
                pc = point(v, u)
                dx, hx = diff(pc, (v, u + radius), (v, u - radius), d[v, u])
                dy, hy = diff(pc, (v + radius, u), (v - radius, u), d[v, u])
                if not hx:
                    cls[v, u] = N.NO_HORIZONTAL
                    continue
                if not hy:
                    cls[v, u] = N.NO_VERTICAL
                    continue
                nx = dy[1] * dx[2] - dy[2] * dx[1]
                ny = dy[2] * dx[0] - dy[0] * dx[2]
                nz = dy[0] * dx[1] - dy[1] * dx[0]
                s = (nx * nx + ny * ny) + nz * nz
                if not (s > 0 and math.isfinite(s)):
                    cls[v, u] = N.DEGENERATE
                    continue
                q = np.sqrt(s)
                n = (nx / q, ny / q, nz / q)
                x, y, zz = pc
                m = np.sqrt((x * x + y * y) + zz * zz)
                cosv = -(((n[0] * x + n[1] * y) + n[2] * zz) / m)
                if not cosv >= min_cos:
                    cls[v, u] = N.GRAZING
                    continue
                assert all(type(a) is F for a in n) and type(cosv) is F
                cls[v, u] = N.USED
                for a in range(3):
                    nrm[a, v, u] = n[a]
                    img[a, v, u] = int(np.rint(n[a] * F(127.5) + F(127.5)))
    return dict(depth=c["depth"], normals=nrm, image=img, count=int((cls == N.USED).sum()), cls=cls)


@pytest.mark.parametrize("name", NAMES)
def test_the_oracle_is_the_header_text_and_the_case_holds_its_classes(name):
    c = C.by_name(name)
    o = N.batch(*c["maps"], **c["kw"])
    hist = np.bincount(o["cls"].ravel(), minlength=6)
    print(f"[normals] {name}: " + ", ".join(f"{N.CLASS_NAMES[k]} {hist[k]}" for k in range(6)))
    for k in c["classes"]:
        assert hist[k] > 0, f"{name} was meant to hold pixels of the class '{N.CLASS_NAMES[k]}'"
    for b in range(len(c["maps"][0])):
        s = _scalar(*[m[b] for m in c["maps"]], **c["kw"])
        assert _bytes(s["cls"]) == _bytes(o["cls"][b])
        assert _bytes(s["depth"]) == _bytes(o["depth"][b, 0]) and _bytes(s["normals"]) == _bytes(o["normals"][b])
        assert _bytes(s["image"]) == _bytes(o["image"][b]) and s["count"] == o["count"][b]
    used = o["cls"] == N.USED
    norm = np.sqrt((o["normals"].astype(np.float64) ** 2).sum(1))
    assert np.abs(norm[used] - 1.0).max(initial=0.0) < 1e-6 and not o["normals"][~np.broadcast_to(used[:, None], o["normals"].shape)].any()
    assert not o["image"][~np.broadcast_to(used[:, None], o["image"].shape)].any()


def test_every_class_and_every_radius_is_exercised():
    seen = set(k for c in C.cases() for k in c["classes"])
    assert seen == set(range(6))
    assert {c["kw"]["radius"] for c in C.cases()} >= {1, 2, 3, 8}
    assert any(c["kw"]["max_jump"] == float("inf") for c in C.cases()) and any(c["kw"].get("filtered") is False for c in C.cases())
    assert any(len(c["maps"][0]) == 2 for c in C.cases())


def test_radius_eight_on_seven_rows_has_no_normal():
    c = C.by_name("r8_seven_rows")
    o = N.batch(*c["maps"], **c["kw"])
    assert o["count"][0] == 0 and not o["normals"].any() and not o["image"].any() and (o["depth"] > 0).all()


def test_the_dyadic_plane_is_exact():
    """z = 2, fx = fy = 64, cx = 33.5, cy = 22.5: every difference is exact, n = (0, 0, -1); rintf(0 * 127.5 + 127.5) = rintf(127.5) = 128 (half
    to even) and rintf(-127.5 + 127.5) = 0"""
    c = C.by_name("dyadic_plane")
    assert (c["kw"]["fx"], c["kw"]["fy"], c["kw"]["cx"], c["kw"]["cy"]) == (64.0, 64.0, 33.5, 22.5)
    o = N.batch(*c["maps"], **c["kw"])
    H, W = c["kw"]["H"], c["kw"]["W"]
    assert o["count"][0] == H * W and (o["depth"] == 2.0).all()
    assert _bytes(o["normals"]) == _bytes(np.broadcast_to(np.array([0.0, 0.0, -1.0], F)[None, :, None, None], (1, 3, H, W)))
    assert _bytes(o["image"]) == _bytes(np.broadcast_to(np.array([128, 128, 0], np.uint8)[None, :, None, None], (1, 3, H, W)))


def test_two_pairs_are_independent():
    c = C.by_name("two_pairs")
    o = N.batch(*c["maps"], **c["kw"])
    own, plane = (N.batch(*C.by_name(n)["maps"], **C.by_name(n)["kw"]) for n in ("own", "dyadic_plane"))
    for k in ("depth", "normals", "image", "count"):
        assert _bytes(o[k][0]) == _bytes(own[k][0]) and _bytes(o[k][1]) == _bytes(plane[k][0])


@pytest.mark.parametrize("cam,pad", [("own", (51, 73)), ("big", (98, 140))])
def test_the_normals_point_to_the_side_of_the_tsdf_gradients(cam, pad):
    """the model poses are the identity, so K26's world-frame gradients are in the camera frame"""
    (disp, occ, conf), kw = TS.live(cam, *pad, pose=tuple(S.IDENTITY))
    o = N.normals(disp, occ, conf, **kw, radius=1, max_jump=1.0, min_cos=0.2)
    _, g, _ = TS.render(cam=cam)
    gn = np.sqrt((g.astype(np.float64) ** 2).sum(0))
    both = (o["cls"] == N.USED) & (gn > 0)
    dot = (o["normals"].astype(np.float64) * g).sum(0)[both] / gn[both]
    print(f"[normals] {cam}: {both.sum()} pixels, dot with the gradients: median {np.median(dot):.4f}, min {dot.min():.3f}")
    assert both.sum() > 1000 and (dot > 0).all()
    assert np.median(dot) > 0.99


WRONG = dict(central_only="central differences only", gate_far="the gate taken against the far neighbour", gate_unscaled="the gate not scaled by radius",
             swapped="dx x dy", no_crop="the crop offset dropped", radius_one="radius ignored", padded_neighbours="padded pixels used as neighbours",
             view_z="the view gate on z alone")


@pytest.mark.parametrize("wrong", list(WRONG))
def test_a_wrong_kernel_is_rejected(wrong):
    rejected = []
    for c in C.cases():
        good, bad = N.batch(*c["maps"], **c["kw"]), N.batch(*c["maps"], **c["kw"], **{wrong: True})
        if any(_bytes(good[k]) != _bytes(bad[k]) for k in ("depth", "normals", "image", "count")):
            rejected.append(c["name"])
    print(f"[normals] {WRONG[wrong]}: rejected by {rejected}")
    assert rejected, f"no case tells the rule from: {WRONG[wrong]}"


def test_frame_to_frame_tracking_through_the_oracles():
    """the model is the normal map of the frame seen from the identity, with identity model poses; the live frame is seen from TRUE; the start
    is the identity.  The condition of test_convergence in test_hip_tsdf_track.py: both pose errors fall to a fifth at the most"""
    (md, mo, mc), mkw = TS.live("own", 51, 73, pose=tuple(S.IDENTITY))
    nm = N.normals(md, mo, mc, **mkw, radius=1, max_jump=1.0, min_cos=0.2)
    (disp, occ, conf), kw = TS.live("own", 51, 73)
    ident = np.array([S.IDENTITY], F)
    o = T.track(disp[None], occ[None], conf[None], ident, ident, nm["depth"][None, None], nm["normals"][None], n_iters=10, **kw, **TS.model_kw(),
                **TS.GATES)
    assert all(it["status"] == 0 for it in o["its"][0])
    r0, t0 = T.pose_errors(S.IDENTITY, TS.TRUE)
    r1, t1 = T.pose_errors(o["poses"][0], TS.TRUE)
    print(f"[normals] frame to frame: rotation {r0:.3g} -> {r1:.3g} (1/{r0 / r1:.0f}), translation {t0:.3g} -> {t1:.3g} (1/{t0 / t1:.0f})")
    assert r1 <= r0 / 5 and t1 <= t0 / 5
