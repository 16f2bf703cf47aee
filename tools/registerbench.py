"""K21 (s2m2_register: the depth map registered to a second camera -- clear, splat with 64-bit atomic minima, resolve) against the same result
composed from torch ops on the device tensors -- the chain in fp32, int64 keys, one ``scatter_reduce_(..., "amin")`` per footprint offset, gathers
for the colours and a scatter for the visibility: what a user writes without K21 -- at 1216x1024 and 2432x2048 with a uint8 image, for splat 1
and 2, for the identity target and the rectified right view, with a tenth of the pixels dropped by the filter and with everything kept
(disparities of 80 .. 280 px, truncation at 10 m).  Same box, same process, alternated, a few repeats each (medians, with the extremes behind
them).

Both sides are timed with events around ``--steps`` replays of a hipGraph that holds one call (neither synchronises).  The three launches of K21
are timed one by one from a torch.profiler pass over eager calls (kernel time on the device, averaged); their sum is below the replay time by the
gaps between the launches.  Bytes: the splat launch reads the three maps and issues one 8-byte atomic per covered footprint pixel; the clear
launch writes 8 bytes per target pixel (and one per source pixel for ``visible``); the resolve launch reads the keys, gathers three colour
bytes per covered pixel and writes 4 + 4 + 3 bytes per target pixel.  With --forward the S forward (fp16, hipGraph replay) and K15 are timed in
the same session at 1216x1024 for the "share of a forward" line.

    python tools/registerbench.py [--steps 200] [--repeats 3] [--forward] [--out profiles/register/registerbench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAL = dict(fx=3896.34, fy=3896.34, cx=1064.836, cy=976.456, baseline=173.557, doffs=163.863)       # Middlebury Bicycle2
CX1 = 1228.699                                                                                      # its cam1
LAUNCHES = ("register_clear_kernel", "register_splat_kernel", "register_resolve_kernel")


def launch_split(fn, calls: int = 20):
    """average device microseconds of K21's three kernels over `calls` eager calls, or None when the profiler reports no kernels"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    out = []
    for name in LAUNCHES:
        total, n = 0.0, 0
        for e in prof.key_averages():
            if name in e.key:
                total += float(getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0))
                n += e.count
        if n == 0:
            return None
        out.append(total / n)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register", "registerbench.txt"))
    a = ap.parse_args()
    import torch
    from s2m2_amd import hip
    from tools.kbench import captured, spread, timed
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    forward_us = k15_us = None
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
    for H, W in ((1024, 1216), (2048, 2432)):
        uu = torch.arange(W, device="cuda", dtype=torch.float32).expand(H, W)
        vv = torch.arange(H, device="cuda", dtype=torch.float32)[:, None].expand(H, W)
        src = torch.arange(H * W, device="cuda", dtype=torch.int64)
        for dropped in ("1/10 dropped", "all kept"):
            g = torch.Generator(device="cuda").manual_seed(H + len(dropped))
            disp = torch.rand((1, 1, H, W), device="cuda", generator=g) * 200.0 + 80.0
            conf = torch.rand((1, 1, H, W), device="cuda", generator=g) * (1.0 if dropped != "all kept" else 0.8) + (0.0 if dropped != "all kept" else 0.2)
            occ = torch.rand((1, 1, H, W), device="cuda", generator=g) * 0.4 + 0.6
            img = torch.randint(0, 256, (1, 3, H, W), device="cuda", dtype=torch.uint8, generator=g)
            if forward_us and H == 1024 and k15_us is None:
                records = torch.empty((1, H * W, 4), device="cuda", dtype=torch.int32)
                cnt = torch.zeros((1,), device="cuda", dtype=torch.int32)
                cws = torch.empty(hip.cloud_workspace_bytes(1, H, W), device="cuda", dtype=torch.uint8)
                gk = captured(lambda: hip.cloud(disp, occ, conf, img, records=records, count=cnt, workspace=cws, **CAL))
                k15_us = statistics.median(timed(gk.replay, a.steps) for _ in range(a.repeats))
                say(f"K15 s2m2_cloud 1216x1024 ({dropped}, same session): {k15_us:.1f} us = {k15_us / forward_us * 100:.2f} % of the S forward")
                del gk, records
            for target in ("identity", "right"):
                cx_t = CAL["cx"] if target == "identity" else CX1
                tx = 0.0 if target == "identity" else -CAL["baseline"] / 1000.0
                for splat in (1, 2):
                    Ht, Wt = H, W
                    out = dict(depth_t=torch.empty((1, 1, Ht, Wt), device="cuda"), index_t=torch.empty((1, 1, Ht, Wt), device="cuda", dtype=torch.int32),
                               image_t=torch.empty((1, 3, Ht, Wt), device="cuda", dtype=torch.uint8),
                               visible=torch.empty((1, 1, H, W), device="cuda", dtype=torch.uint8), count=torch.empty((1,), device="cuda", dtype=torch.int32))
                    ws = torch.empty(hip.register_workspace_bytes(1, Ht, Wt), device="cuda", dtype=torch.uint8)
                    kw = dict(Ht=Ht, Wt=Wt, splat=splat, fx_t=CAL["fx"], fy_t=CAL["fy"], cx_t=cx_t, cy_t=CAL["cy"], R=[1, 0, 0, 0, 1, 0, 0, 0, 1],
                              t=[tx, 0.0, 0.0], workspace=ws, depth_trunc=10.0, **out, **CAL)

                    def k21():
                        hip.register(disp, occ, conf, img, **kw)

                    c = (splat - 2) / 2.0
                    big = torch.iinfo(torch.int64).max
                    # constants as device tensors, made outside the captured region
                    big_t, minus_one = (torch.tensor(x, device="cuda", dtype=torch.int64) for x in (big, -1))
                    zero_f, minus_one_f, far = (torch.tensor(x, device="cuda", dtype=torch.float32) for x in (0.0, -1.0, 1e9))
                    zero_b = torch.zeros((), device="cuda", dtype=torch.uint8)
                    spread_idx = src % (H * W) if Ht * Wt == H * W else torch.arange(Ht * Wt, device="cuda") % (H * W)

                    def composed():
                        valid = (conf[0, 0] > 0.1) & (occ[0, 0] > 0.5)
                        d = torch.where(valid, disp[0, 0], minus_one_f)
                        z = torch.where(d <= 0, far, bf / (d + doffs)) / 1000.0
                        keep = (z > 0) & (z < 10.0)                            # every disparity here is nearer; the filter's sentinel is not
                        x = (uu - CAL["cx"]) * z / CAL["fx"]
                        y = (vv - CAL["cy"]) * z / CAL["fy"]
                        X, Y, Z = x + tx, y, z                                   # R = I: what a user writes for these two targets
                        ok = keep & (Z > 0) & torch.isfinite(Z)
                        fu = torch.floor(CAL["fx"] * X / Z + cx_t - c).to(torch.int64)
                        fv = torch.floor(CAL["fy"] * Y / Z + CAL["cy"] - c).to(torch.int64)
                        key = (Z.view(torch.int32).to(torch.int64) << 32) | src.view(H, W)
                        zbuf = torch.full((Ht * Wt,), big, device="cuda", dtype=torch.int64)
                        for dy in range(splat):
                            for dx in range(splat):
                                tu, tv = fu + dx, fv + dy
                                m = ok & (tu >= 0) & (tu < Wt) & (tv >= 0) & (tv < Ht)
                                # what misses keeps a slot inside the buffer and offers the largest key: no effect, and no word everyone meets on
                                zbuf.scatter_reduce_(0, (tv * Wt + tu).clamp(0, Ht * Wt - 1).reshape(-1), torch.where(m, key, big_t).reshape(-1), "amin")
                        hit = zbuf != big
                        depth = torch.where(hit, (zbuf >> 32).to(torch.int32).view(torch.float32), zero_f)
                        index = torch.where(hit, zbuf & 0xFFFFFFFF, minus_one)
                        colour = torch.where(hit, img[0].reshape(3, -1)[:, index.clamp(min=0)], zero_b)
                        visible = torch.zeros((H * W,), device="cuda", dtype=torch.uint8)
                        visible.scatter_reduce_(0, torch.where(hit, index, spread_idx), hit.to(torch.uint8), "amax")       # holes: a slot each
                        return depth, index.to(torch.int32), colour, visible, hit.sum()

                    g21 = captured(k21)
                    try:
                        gt, how = captured(composed), "hipGraph replay"
                        run_t = gt.replay
                    except Exception as e:  # noqa: BLE001  (an op that cannot be captured on this torch)
                        torch.cuda.synchronize()
                        gt, how, run_t = None, f"eager ({type(e).__name__} under capture)", composed
                    t_k21, t_torch = [], []
                    for _ in range(a.repeats):                               # alternated
                        t_k21.append(timed(g21.replay, a.steps))
                        t_torch.append(timed(run_t, max(10, a.steps // 4)))
                    n = int(out["count"][0])
                    ref = composed()
                    # the composition is not the oracle (tests/test_hip_register.py has one): torch picks its own operation order
                    assert abs(int(ref[4]) - n) <= max(8, n // 1000), (int(ref[4]), n)
                    kept = int(((conf > 0.1) & (occ > 0.5)).sum())                  # an upper bound of the atomics: footprints that leave the target issue none
                    us, ut = statistics.median(t_k21), statistics.median(t_torch)
                    split = launch_split(k21)
                    atom = 8 * kept * splat * splat
                    moved = 8 * Ht * Wt + H * W + 3 * 4 * H * W + atom + 8 * Ht * Wt + 3 * n + 11 * Ht * Wt + n
                    say(f"{W}x{H} {dropped}, {target} target, splat {splat}: {n / (Ht * Wt):.3f} of the target covered")
                    say(f"    K21 s2m2_register   {spread(t_k21)}   {moved / 1e6:6.1f} MB moved, {atom / 1e6:5.1f} MB of them as atomics"
                        + (f"   {us / forward_us * 100:.2f} % of the S forward" if forward_us and H == 1024 else ""))
                    say(f"    torch composition   {spread(t_torch)}   {ut / us:5.1f}x K21   ({how})")
                    if split:
                        say(f"    launches (device time, eager): clear {split[0]:.1f} us, splat {split[1]:.1f} us = {atom / split[1] / 1e6:.2f} TB/s of atomic bytes, "
                            f"resolve {split[2]:.1f} us")
                    else:
                        say("    launches: the profiler reported no kernels")
                    del g21, gt

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
