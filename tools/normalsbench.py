"""K28 (s2m2_normals: the normal map of the disparity map, one launch plus the clear of count) against (a) the same maps composed from torch ops on
the device tensors -- the chain in fp32, shifted copies (torch.roll) with border masks, ``where`` for the one-sided differences, ``cross`` --:
what a user writes without K28, and (b) K15 alone on the same maps (the dense depth, and the whole cloud), at 1216x1024 and 2432x2048, for
radius 1 and 4, with all four outputs and with the normals alone.  The scene is a smooth surface (disparities of 80 .. 280 px, truncation at
10 m) with a tenth of the pixels dropped by the filter.  Same box, same process, alternated, a few repeats each (medians, with the extremes
behind them).

Both sides are timed with events around ``--steps`` replays of a hipGraph that holds one call (neither synchronises).  Bytes: K28 must read the
three maps (12 B per pixel) and write what is requested (depth 4, normals 12, image 3 B per pixel); the floor is that traffic at the 6.29 TB/s
copy rate the project uses.  The composition's result is compared first: torch picks its own operation order and division, so the comparison
reports the pixels whose hole state differs and the largest difference of a component instead of demanding bytes
(tests/test_hip_normals.py holds K28 to the oracle's bytes).  ``cloud.track`` of 10 iterations against a NormalMap (K27's two launches per
iteration on a model without a volume) is timed at both sizes for the line beside profiles/tsdf/tsdftrack.txt.  With --forward the S forward
(fp16, hipGraph replay) is timed in the same session at 1216x1024 for the "share of a forward" figures.

The library is the one S2M2_LIB_SUFFIX names: a build with S2M2_BUILD_DEFINES=-DS2M2_NORMALS_LDS=0 gives the form without LDS (--label names
it in the output).

    python tools/normalsbench.py [--steps 200] [--repeats 3] [--forward] [--label TEXT] [--out profiles/normals/normalsbench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAL = dict(fx=3896.34, fy=3896.34, cx=1064.836, cy=976.456, baseline=173.557, doffs=163.863)       # Middlebury Bicycle2
COPY_TBS = 6.29
OUT_BYTES = dict(depth=4, normals=12, image=3, count=0)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--label", default="LDS tile with a halo (the default build)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition and K15 (a second form of K28 is timed against the first)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals", "normalsbench.txt"))
    a = ap.parse_args()
    import torch
    from s2m2_amd import cloud, hip
    from tools.kbench import captured, spread, timed
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    say(f"K28 s2m2_normals: {a.label}")
    forward_us = None
    if a.forward:
        from s2m2_amd.model import build_model
        from s2m2_amd.spec import MODEL_CONFIGS
        from s2m2_amd.weights import seeded_state_dict, synthetic_pair
        C, ntr = MODEL_CONFIGS["S"]
        m = build_model("S")
        m.load_state_dict(seeded_state_dict(C, 1, ntr, 0), strict=True)
        m = m.cuda().eval()
        l, r = (t.cuda().contiguous() for t in synthetic_pair(1024, 1216, 1, 32, 0))
        with torch.autocast("cuda", dtype=torch.float16):
            for _ in range(3):
                m(l, r)
            forward_us = statistics.median(timed(lambda: m(l, r), 50) for _ in range(a.repeats))
        say(f"S forward 1216x1024 fp16 (hipGraph replay, same session): {forward_us / 1000.0:.3f} ms")
        del m

    bf, doffs = float(CAL["baseline"] * CAL["fx"]), CAL["doffs"]
    kcam = dict(depth_trunc=10.0, **CAL)
    for H, W in ((1024, 1216), (2048, 2432)):
        uu = torch.arange(W, device="cuda", dtype=torch.float32).expand(H, W)
        vv = torch.arange(H, device="cuda", dtype=torch.float32)[:, None].expand(H, W)
        g = torch.Generator(device="cuda").manual_seed(H)
        disp = (180.0 + 60.0 * torch.sin(uu / 97.0) + 40.0 * torch.cos(vv / 71.0))[None, None].contiguous()
        conf = torch.rand((1, 1, H, W), device="cuda", generator=g)
        occ = torch.rand((1, 1, H, W), device="cuda", generator=g) * 0.4 + 0.6
        img = torch.randint(0, 256, (1, 3, H, W), device="cuda", dtype=torch.uint8, generator=g)
        outs = dict(depth=torch.empty((1, 1, H, W), device="cuda"), normals=torch.empty((1, 3, H, W), device="cuda"),
                    image=torch.empty((1, 3, H, W), device="cuda", dtype=torch.uint8), count=torch.empty((1,), device="cuda", dtype=torch.int32))
        say(f"{W}x{H}, 1/10 dropped by the filter")
        if not a.no_torch:
            depth15 = torch.empty((1, 1, H, W), device="cuda")
            records = torch.empty((1, H * W, 4), device="cuda", dtype=torch.int32)
            cnt = torch.zeros((1,), device="cuda", dtype=torch.int32)
            cws = torch.empty(hip.cloud_workspace_bytes(1, H, W), device="cuda", dtype=torch.uint8)
            gd = captured(lambda: hip.cloud(disp, occ, conf, img, depth=depth15, **kcam))
            gc = captured(lambda: hip.cloud(disp, occ, conf, img, records=records, count=cnt, workspace=cws, **kcam))
            td = [timed(gd.replay, a.steps) for _ in range(a.repeats)]
            tc = [timed(gc.replay, a.steps) for _ in range(a.repeats)]
            say(f"    K15 s2m2_cloud, depth only (one launch)   {spread(td)}   floor {16 * H * W / COPY_TBS / 1e6:5.1f} us")
            say(f"    K15 s2m2_cloud, the cloud (two launches)  {spread(tc)}")
            del gd, gc, records

        zero_f, minus_one_f, far = (torch.tensor(x, device="cuda", dtype=torch.float32) for x in (0.0, -1.0, 1e9))
        zero_b = torch.zeros((), device="cuda", dtype=torch.uint8)
        for radius in (1, 4):
            gate, min_cos = 1.0 * radius, 0.0
            inside = {}
            for name, (dv, du) in dict(hp=(0, radius), hm=(0, -radius), vp=(radius, 0), vm=(-radius, 0)).items():
                inside[name] = ((vv + dv >= 0) & (vv + dv < H) & (uu + du >= 0) & (uu + du < W), (-dv, -du))

            def composed():
                d0 = disp[0, 0]
                valid = (conf[0, 0] > 0.1) & (occ[0, 0] > 0.5)
                d = torch.where(valid, d0, minus_one_f)
                z = torch.where(d <= 0, far, bf / (d + doffs)) / 1000.0
                keep = (z > 0) & (z < 10.0)
                z = torch.where(keep, z, zero_f)
                P = torch.stack([(uu - CAL["cx"]) * z / CAL["fx"], (vv - CAL["cy"]) * z / CAL["fy"], z])

                def side(name):
                    ins, sh = inside[name]
                    use = ins & torch.roll(keep, sh, (0, 1)) & ((torch.roll(d0, sh, (0, 1)) - d0).abs() <= gate)
                    return torch.where(use, torch.roll(P, sh, (1, 2)), P), use

                (ap_, up), (am, um) = side("hp"), side("hm")
                (bp, vp_), (bm, vm_) = side("vp"), side("vm")
                n = torch.cross(bp - bm, ap_ - am, dim=0)
                s = (n * n).sum(0)
                n = n / s.sqrt()
                cosv = -(n * P).sum(0) / (P * P).sum(0).sqrt()
                used = keep & (up | um) & (vp_ | vm_) & (s > 0) & torch.isfinite(s) & (cosv >= min_cos)
                normals = torch.where(used, n, zero_f)
                image = torch.where(used, torch.round(n * 127.5 + 127.5).to(torch.uint8), zero_b)
                return z, normals, image, used.sum()

            for which in (("depth", "normals", "image", "count"), ("normals",)):
                kw = dict(H=H, W=W, radius=radius, max_jump=1.0, min_cos=min_cos, **kcam, **{k: outs[k] for k in which})
                g28 = captured(lambda: hip.normals(disp, occ, conf, **kw))
                t28 = [timed(g28.replay, a.steps) for _ in range(a.repeats)]
                moved = (12 + sum(OUT_BYTES[k] for k in which)) * H * W
                floor = moved / COPY_TBS / 1e6
                us = statistics.median(t28)
                say(f"    K28 radius {radius}, {'all outputs' if len(which) == 4 else 'normals only'}:   {spread(t28)}   {moved / 1e6:6.1f} MB mandatory = "
                    f"{floor:5.1f} us at {COPY_TBS} TB/s: {floor / us * 100:4.1f} % of the copy rate"
                    + (f"   {us / forward_us * 100:.2f} % of the S forward" if forward_us and H == 1024 else ""))
                del g28
            if a.no_torch:
                continue
            hip.normals(disp, occ, conf, H=H, W=W, radius=radius, max_jump=1.0, min_cos=min_cos, **kcam, **outs)
            ref = composed()
            torch.cuda.synchronize()
            n28, nt = int(outs["count"][0]), int(ref[3])
            has28, hast = (outs["normals"][0] != 0).any(0), (ref[1] != 0).any(0)
            both = has28 & hast
            diff = float((outs["normals"][0] - ref[1]).abs().amax(0)[both].max())
            say(f"    torch composition, radius {radius}: {nt} normals against K28's {n28}; hole state differs at {int((has28 != hast).sum())} pixels; "
                f"largest difference of a component where both exist {diff:.3g}; depth equal: {bool(torch.equal(outs['depth'][0, 0], ref[0]))}")
            assert abs(nt - n28) <= max(8, n28 // 1000), (nt, n28)
            try:
                gt, how = captured(composed), "hipGraph replay"
                run_t = gt.replay
            except Exception as e:  # noqa: BLE001  (an op that cannot be captured on this torch)
                torch.cuda.synchronize()
                gt, how, run_t = None, f"eager ({type(e).__name__} under capture)", composed
            tt = [timed(run_t, max(10, a.steps // 4)) for _ in range(a.repeats)]
            say(f"    torch composition, radius {radius}        {spread(tt)}   ({how})")
            del gt

        # cloud.track: ten iterations of K27 against the NormalMap of the same maps, from the identity
        nm = cloud.normals(disp, occ, conf, H=H, W=W, fx=CAL["fx"], cx=CAL["cx"], cy=CAL["cy"], baseline=CAL["baseline"], doffs=CAL["doffs"],
                           depth_trunc=10.0, min_cos=0.2, want_count=False)
        pbuf = torch.eye(3, 4, device="cuda").reshape(1, 12).contiguous()
        ws = torch.empty((hip.tsdf_track_workspace_bytes(1, H, W) // 8,), device="cuda", dtype=torch.float64)
        systems = torch.empty((1, 10, 32), device="cuda", dtype=torch.float64)
        tkw = dict(H=H, W=W, mfx=CAL["fx"], mfy=CAL["fy"], mcx=CAL["cx"], mcy=CAL["cy"], max_dist=0.05, min_count=100, max_rot=0.2, max_trans=0.2,
                   n_iters=10, workspace=ws, systems=systems, **kcam)
        gtr = captured(lambda: hip.tsdf_track(disp, occ, conf, pbuf, nm.poses, nm.depth, nm.gradients_buf, **tkw))
        ttr = [timed(gtr.replay, max(10, a.steps // 4)) for _ in range(a.repeats)]
        row = systems[0, -1].cpu()
        say(f"    cloud.track, 10 iterations against the NormalMap   {spread(ttr)}   = {statistics.median(ttr) / 10:.1f} us per iteration; "
            f"last iteration: {int(row[28])} correspondences, status {int(row[29])}")
        del gtr

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
