"""K29 (s2m2_smooth: edge-preserving smoothing of the disparity map, one launch plus the clear of count) against (a) the same map composed from
torch ops on the device tensors -- K15's keep in fp32, one shifted slice of the NaN-padded map per tap, ``exp`` for the range weight --: what a
user writes without K29, and (b) K28's launch (all outputs, radius 1) on the same maps, at 1216x1024 and 2432x2048, for radius 1, 2, 3, 5 and 8
with disp_out and count (taps adds 4 B per pixel and is timed once per size).  The scene is a smooth surface (disparities of 80 .. 280 px,
truncation at 10 m) with Gaussian disparity noise of 0.2 px and a tenth of the pixels dropped by the filter; sigma_s = radius / 2, sigma_r =
0.5 px, max_jump = 2 px.  Same box, same process, alternated, a few repeats each (medians, with the extremes behind them).

Both sides are timed with events around ``--steps`` replays of a hipGraph that holds one call (neither synchronises).  Bytes: K29 must read the
three maps (12 B per pixel) and write what is requested (disp_out 4, taps 4 B per pixel); the floor is that traffic at the 6.29 TB/s copy rate
the project uses.  The kernel is not expected at that floor: it evaluates (2 radius + 1)^2 taps per pixel out of LDS, so the taps per second
are reported beside it.  The composition's result is compared first: torch evaluates ``exp`` where K29 reads a table of 257 entries, so the
comparison reports the largest difference instead of demanding bytes (tests/test_hip_smooth.py holds K29 to the oracle's bytes).  With
--forward the S forward (fp16, hipGraph replay) is timed in the same session at 1216x1024 for the "share of a forward" figures.

The library is the one S2M2_LIB_SUFFIX names: a build with S2M2_BUILD_DEFINES=-DS2M2_SMOOTH_WR_LDS=0 reads the range table from the kernel
arguments instead of LDS (--label names it in the output; --no-torch --append adds its K29 lines to the file of the default build).

    python tools/smoothbench.py [--steps 200] [--repeats 3] [--forward] [--label TEXT] [--no-torch] [--append] [--out profiles/smooth/smoothbench.txt]
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAL = dict(fx=3896.34, fy=3896.34, cx=1064.836, cy=976.456, baseline=173.557, doffs=163.863)       # Middlebury Bicycle2
COPY_TBS = 6.29
RADII = (1, 2, 3, 5, 8)
SIGMA_R, MAX_JUMP = 0.5, 2.0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--label", default="range table in LDS (the default build)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition and K28 (a second form of K29 is timed against the first)")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth", "smoothbench.txt"))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from s2m2_amd import hip
    from tools.kbench import captured, spread, timed
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    say(f"K29 s2m2_smooth: {a.label}")
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
        disp = (180.0 + 60.0 * torch.sin(uu / 97.0) + 40.0 * torch.cos(vv / 71.0) + 0.2 * torch.randn((H, W), device="cuda", generator=g))[None, None].contiguous()
        conf = torch.rand((1, 1, H, W), device="cuda", generator=g)
        occ = torch.rand((1, 1, H, W), device="cuda", generator=g) * 0.4 + 0.6
        out = torch.empty((1, 1, H, W), device="cuda")
        taps = torch.empty((1, 1, H, W), device="cuda", dtype=torch.int32)
        count = torch.empty((1,), device="cuda", dtype=torch.int32)
        say(f"{W}x{H}, noise 0.2 px, 1/10 dropped by the filter, sigma_s = radius / 2, sigma_r = {SIGMA_R}, max_jump = {MAX_JUMP}")
        if not a.no_torch:
            o28 = dict(depth=torch.empty((1, 1, H, W), device="cuda"), normals=torch.empty((1, 3, H, W), device="cuda"),
                       image=torch.empty((1, 3, H, W), device="cuda", dtype=torch.uint8), count=torch.empty((1,), device="cuda", dtype=torch.int32))
            g28 = captured(lambda: hip.normals(disp, occ, conf, H=H, W=W, radius=1, max_jump=1.0, min_cos=0.0, **kcam, **o28))
            t28 = [timed(g28.replay, a.steps) for _ in range(a.repeats)]
            say(f"    K28 s2m2_normals, radius 1, all outputs (one launch)   {spread(t28)}")
            del g28, o28
        minus_one, far, nan = (torch.tensor(x, device="cuda", dtype=torch.float32) for x in (-1.0, 1e9, float("nan")))
        zero = torch.zeros((), device="cuda")

        for radius in RADII:
            rule = dict(radius=radius, sigma_s=radius / 2.0, sigma_r=SIGMA_R, max_jump=MAX_JUMP)
            ws = [math.exp(-(k * k) / (2.0 * (radius / 2.0) ** 2)) for k in range(radius + 1)]

            def composed():
                d0 = disp[0, 0]
                valid = (conf[0, 0] > 0.1) & (occ[0, 0] > 0.5)
                d = torch.where(valid, d0, minus_one)
                z = torch.where(d <= 0, far, bf / (d + doffs)) / 1000.0
                keep = (z > 0) & (z < 10.0)
                pad = F.pad(torch.where(keep, d0, nan), (radius, radius, radius, radius), value=float("nan"))
                num, den = torch.zeros_like(d0), torch.zeros_like(d0)
                for dv in range(-radius, radius + 1):
                    for du in range(-radius, radius + 1):
                        e = pad[radius + dv:radius + dv + H, radius + du:radius + du + W] - d0
                        ok = e.abs() <= MAX_JUMP                                  # a NaN fails
                        w = torch.where(ok, (ws[abs(dv)] * ws[abs(du)]) * torch.exp(e * e * (-0.5 / SIGMA_R ** 2)), zero)
                        num = num + torch.where(ok, w * e, zero)
                        den = den + w
                return torch.where(keep, d0 + num / den, minus_one), keep.sum()

            kw = dict(H=H, W=W, **rule, **kcam)
            g29 = captured(lambda: hip.smooth(disp, occ, conf, disp_out=out, count=count, **kw))
            t29 = [timed(g29.replay, a.steps) for _ in range(a.repeats)]
            hip.smooth(disp, occ, conf, disp_out=out, taps=taps, count=count, **kw)
            torch.cuda.synchronize()
            n_taps, kept = int(taps.sum(dtype=torch.int64)), int(count[0])
            us = statistics.median(t29)
            floor = 16 * H * W / COPY_TBS / 1e6
            say(f"    K29 radius {radius}, disp_out + count:   {spread(t29)}   {16 * H * W / 1e6:6.1f} MB mandatory = {floor:5.1f} us at {COPY_TBS} TB/s: "
                f"{floor / us * 100:4.1f} % of the copy rate;   {n_taps / 1e6:7.1f} M taps = {n_taps / us / 1e6:6.2f} T taps/s"
                + (f"   {us / forward_us * 100:.2f} % of the S forward" if forward_us and H == 1024 else ""))
            del g29
            if radius == 3:
                g29 = captured(lambda: hip.smooth(disp, occ, conf, disp_out=out, taps=taps, count=count, **kw))
                tt = [timed(g29.replay, a.steps) for _ in range(a.repeats)]
                say(f"    K29 radius {radius}, all three outputs:  {spread(tt)}   (taps: 4 B per pixel more)")
                del g29
            if a.no_torch:
                continue
            ref, nref = composed()
            torch.cuda.synchronize()
            k = out[0, 0] != -1
            diff = float((out[0, 0] - ref)[k].abs().max())
            say(f"    torch composition, radius {radius}: {int(nref)} kept against K29's {kept}; kept set equal: {bool(torch.equal(k, ref != -1))}; "
                f"largest difference of a smoothed disparity {diff:.3g} px (exp against the 257-entry table)")
            try:
                gt, how = captured(composed), "hipGraph replay"
                run_t = gt.replay
            except Exception as e:  # noqa: BLE001  (an op that cannot be captured on this torch)
                torch.cuda.synchronize()
                gt, how, run_t = None, f"eager ({type(e).__name__} under capture)", composed
            tt = [timed(run_t, max(3, a.steps // (4 * (2 * radius + 1)))) for _ in range(a.repeats)]
            say(f"    torch composition, radius {radius}        {spread(tt)}   ({how}; {statistics.median(tt) / us:.0f}x K29)")
            del gt

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(("\n" if a.append else "") + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
