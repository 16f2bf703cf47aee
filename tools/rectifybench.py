"""K16 (s2m2_rectify: inverse map through the distortion model + bilinear gather, one launch per population) against the same result composed
from torch ops on the device -- the maps in torch, then F.grid_sample(mode="bilinear", padding_mode="zeros", align_corners=True) -- at the
reference rig's 2048x1536, for N = 1 and N = 21 samples x 2 cameras, fp32 and uint8 output, both block orders.  Same box, same process,
alternated, a few repeats each (medians).

Both are timed with events around `--steps` replays of a hipGraph that holds one call.  Bytes moved by K16, counted as in DESIGN.md (K16): every
output element written once, each source image read once; the fraction is of the 8 TB/s HBM peak.  With --forward the S forward (fp16, hipGraph
replay, batch 1) is timed in the same session at 2048x1536 for the share of one CEM iteration (N rectified pairs + N scoring forwards).

    python tools/rectifybench.py [--steps 50] [--repeats 3] [--forward] [--out profiles/rectify/rectifybench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify", "rectifybench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from s2m2_amd import hip, rectify
    from tools.kbench import captured, timed
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    W, H = 2048, 1536
    forward_us = None
    if a.forward:
        from s2m2_amd.model import build_model
        from s2m2_amd.spec import MODEL_CONFIGS
        from s2m2_amd.weights import seeded_state_dict, synthetic_pair
        C, ntr = MODEL_CONFIGS["S"]
        m = build_model("S")
        m.load_state_dict(seeded_state_dict(C, 1, ntr, 0), strict=True)
        m = m.cuda().eval()
        l, r = (t.cuda().contiguous() for t in synthetic_pair(H, W, 1, 32, 0))
        with torch.autocast("cuda", dtype=torch.float16):
            for _ in range(3):
                m(l, r)
            forward_us = statistics.median(timed(lambda: m(l, r), 10) for _ in range(a.repeats))
        say(f"S forward 2048x1536 fp16, one pair (hipGraph replay, same session): {forward_us / 1000.0:.3f} ms")
        del m, l, r

    calib = rectify.parse_xml_calibration(os.path.join(ROOT, "tests", "golden", "calib_head.xml"))
    g = torch.Generator(device="cuda").manual_seed(0)
    srcs = [torch.randint(0, 256, (H, W, 3), device="cuda", dtype=torch.uint8, generator=g) for _ in range(2)]
    planar = torch.stack([s.permute(2, 0, 1).float() for s in srcs])                    # (2,3,H,W) fp32 for grid_sample
    vv, uu = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    rng = np.random.RandomState(0)
    for N in (1, 21):
        deltas = np.concatenate([np.zeros((1, 3)), rng.normal(0, 0.002, (N - 1, 3))])
        rec = torch.from_numpy(rectify.population_records(calib, (W, H), deltas).astype(np.float32)).cuda()
        n_img = 2 * N
        for dtype in (torch.float32, torch.uint8):
            out = torch.empty((n_img, 3, H, W), device="cuda", dtype=dtype)
            graphs = {name: captured(lambda o=order: hip.rectify(srcs, rec, out, order=o))
                      for name, order in (("sample-fastest", hip.RECTIFY_ORDER_SAMPLE), ("tile-fastest", hip.RECTIFY_ORDER_TILE))}
            ref = torch.empty((n_img, 3, H, W), device="cuda", dtype=dtype)

            def composed():
                for i in range(n_img):                                           # one image at a time: the grid of 42 images would be 1 GB
                    r = rec[i]
                    X = r[1] * uu + r[2] * vv + r[3]
                    Y = r[4] * uu + r[5] * vv + r[6]
                    Wh = r[7] * uu + r[8] * vv + r[9]
                    x, y = X / Wh, Y / Wh
                    r2 = x * x + y * y
                    kr = 1 + r[14] * r2 + r[15] * r2 * r2 + r[18] * r2 * r2 * r2
                    mx = r[10] * (x * kr + 2 * r[16] * x * y + r[17] * (r2 + 2 * x * x)) + r[12]
                    my = r[11] * (y * kr + r[16] * (r2 + 2 * y * y) + 2 * r[17] * x * y) + r[13]
                    grid = torch.stack([mx * (2.0 / (W - 1)) - 1.0, my * (2.0 / (H - 1)) - 1.0], dim=-1)[None]
                    o = F.grid_sample(planar[i // N:i // N + 1], grid, mode="bilinear", padding_mode="zeros", align_corners=True)
                    ref[i] = torch.round(o[0]) if dtype == torch.float32 else torch.round(o[0]).clamp(0, 255).to(torch.uint8)

            gt = captured(composed)
            t = {k: [] for k in list(graphs) + ["torch"]}
            for _ in range(a.repeats):                                           # alternated
                for k, gr in graphs.items():
                    t[k].append(timed(gr.replay, a.steps))
                t["torch"].append(timed(gt.replay, max(3, a.steps // 10)))
            graphs["sample-fastest"].replay()
            gt.replay()
            torch.cuda.synchronize()
            d = (out[::max(1, n_img // 4)].float() - ref[::max(1, n_img // 4)].float()).abs()
            assert float(d.max()) <= 1.0 and float((d != 0).float().mean()) < 0.05, (float(d.max()), float((d != 0).float().mean()))
            med = {k: statistics.median(v) for k, v in t.items()}
            moved = n_img * 3 * H * W * out.element_size() + 2 * 3 * H * W
            best = min(med["sample-fastest"], med["tile-fastest"])
            line = (f"2048x1536 N={N:2d} x 2 cameras {str(dtype).split('.')[1]:7s}: K16 sample-fastest {med['sample-fastest']:8.1f} us  tile-fastest "
                    f"{med['tile-fastest']:8.1f} us   torch composition {med['torch']:9.1f} us   ratio {med['torch'] / med['sample-fastest']:5.1f}x   "
                    f"{moved / 1e6:7.1f} MB moved = {moved / med['sample-fastest'] / 1e6:5.2f} TB/s = {moved / med['sample-fastest'] / 1e6 / 8.0 * 100:4.1f} % of 8 TB/s"
                    f" (best order {moved / best / 1e6 / 8.0 * 100:4.1f} %)")
            if forward_us:
                line += f"   rectification is {med['sample-fastest'] / (med['sample-fastest'] + N * forward_us) * 100:.2f} % of rectify + {N} scoring forwards"
            say(line)
            del graphs, gt, out, ref

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
