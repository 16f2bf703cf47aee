"""K15 (s2m2_cloud: filter + depth + compacted point cloud, two launches) against the same result composed from torch ops on the device tensors
-- mask, where, divide, nonzero, gather, stack: the reference's host method moved to the GPU, what a user writes without K15 -- at 1216x1024
and 2432x2048 with a uint8 image and a kept share near 1/3 and near 1.  Same box, same process, alternated, a few repeats each (medians).

K15 is timed with events around `--steps` replays of a hipGraph that holds one call; the torch composition cannot be captured (nonzero
synchronises) and is timed with events around `--steps` eager calls.  Bytes moved by K15, counted as in DESIGN.md (K15): launch A reads the three
maps, launch B reads them again plus the image, and writes 16 bytes per kept pixel; the fraction is of 8 TB/s.  With --forward the S forward
(fp16, hipGraph replay) is timed in the same session at 1216x1024 for the "share of a forward" line.

    python tools/cloudbench.py [--steps 200] [--repeats 3] [--forward] [--out profiles/cloud/cloudbench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAL = dict(fx=3896.34, fy=3896.34, cx=1064.836, cy=976.456, baseline=173.557, doffs=163.863)       # Middlebury Bicycle2


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud", "cloudbench.txt"))
    a = ap.parse_args()
    import torch
    from s2m2_amd import hip
    from tools.kbench import captured, timed
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

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

    for H, W in ((1024, 1216), (2048, 2432)):
        for share in ("1/3", "1"):
            g = torch.Generator(device="cuda").manual_seed(H + len(share))
            if share == "1":
                disp = torch.rand((1, 1, H, W), device="cuda", generator=g) * 200.0 + 80.0
                conf = torch.rand((1, 1, H, W), device="cuda", generator=g) * 0.8 + 0.2
                occ = torch.rand((1, 1, H, W), device="cuda", generator=g) * 0.4 + 0.6
            else:
                disp = torch.rand((1, 1, H, W), device="cuda", generator=g) * 320.0 - 20.0
                conf = torch.rand((1, 1, H, W), device="cuda", generator=g)
                occ = torch.rand((1, 1, H, W), device="cuda", generator=g)
            img = torch.randint(0, 256, (1, 3, H, W), device="cuda", dtype=torch.uint8, generator=g)
            records = torch.empty((1, H * W, 4), device="cuda", dtype=torch.int32)
            count = torch.zeros((1,), device="cuda", dtype=torch.int32)
            ws = torch.empty(hip.cloud_workspace_bytes(1, H, W), device="cuda", dtype=torch.uint8)
            kw = dict(depth_trunc=3.0, records=records, count=count, workspace=ws, **CAL)

            def k15():
                hip.cloud(disp, occ, conf, img, **kw)

            graph = captured(k15)

            bf, doffs = float(CAL["baseline"] * CAL["fx"]), CAL["doffs"]
            uu = torch.arange(W, device="cuda", dtype=torch.float32).expand(H, W)
            vv = torch.arange(H, device="cuda", dtype=torch.float32)[:, None].expand(H, W)

            def composed():
                valid = (conf[0, 0] > 0.1) & (occ[0, 0] > 0.5)
                d = torch.where(valid, disp[0, 0], -1.0)
                z = torch.where(d <= 0, 1e9, bf / (d + doffs)) / 1000.0
                idx = torch.nonzero(((z > 0) & (z < 3.0)).reshape(-1)).squeeze(1)         # synchronises
                zk = z.reshape(-1)[idx]
                x = (uu.reshape(-1)[idx] - CAL["cx"]) * zk / CAL["fx"]
                y = (vv.reshape(-1)[idx] - CAL["cy"]) * zk / CAL["fy"]
                return torch.stack([x, y, zk], dim=1), img[0].reshape(3, -1)[:, idx].t().contiguous()

            t_k15, t_torch = [], []
            for _ in range(a.repeats):                               # alternated
                t_k15.append(timed(graph.replay, a.steps))
                t_torch.append(timed(composed, max(10, a.steps // 4)))
            n = int(count[0])
            pts, _ = composed()
            # the composition is not the oracle (tests/test_hip_cloud.py is): torch evaluates the chain in its own operation order, so a pixel
            # whose z rounds onto the truncation threshold may fall on the other side
            assert abs(pts.shape[0] - n) <= 8, (pts.shape, n)
            us, ut = statistics.median(t_k15), statistics.median(t_torch)
            moved = 2 * 3 * 4 * H * W + 3 * H * W + 16 * n
            say(f"{W}x{H} kept {n / (H * W):.3f}: K15 {us:8.1f} us   torch composition {ut:8.1f} us   ratio {ut / us:5.1f}x   "
                f"{moved / 1e6:6.1f} MB moved = {moved / us / 1e6 / 8.0 * 100:4.1f} % of 8 TB/s"
                + (f"   {us / forward_us * 100:.2f} % of the S forward" if forward_us and H == 1024 else ""))
            del graph

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
