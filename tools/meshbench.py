"""K20 (s2m2_mesh: K15's vertices + the faces between neighbouring kept pixels, three launches) against its two yardsticks, same box, same
process, alternated: the same result composed from torch ops on the device tensors (masks, shifted comparisons, cumsum ranks, nonzero, gathers:
what a user writes without K20) and K15 (s2m2_cloud) alone on the same inputs -- at 1216x1024 and 2432x2048 with a uint8 image, on a
piecewise-planar scene with a tenth of the pixels dropped and on a constant scene where every pixel is kept and every quad gives two faces.

K20 and K15 are timed with events around `--steps` replays of a hipGraph that holds one call; the torch composition cannot be captured (nonzero
synchronises) and is timed with events around `--steps // 4` (at least 20) eager calls.  Every figure is the median of `--repeats` alternated
windows with their minimum and maximum behind it.  Bytes: the MANDATORY traffic of each stage -- every input read once, every output written
once: the three maps (12 B per pixel), the image (3 B per pixel), 16 B per vertex, and for K20 12 B per face -- over the measured time, as a
rate and as a fraction of 8 TB/s.  K20's own traffic is larger (the maps are read twice and disp a third time, the rank map is
written and read); the mandatory figure is the one that compares with K15's.  With --forward the S forward (fp16, hipGraph replay) is timed in
the same session at 1216x1024 for the "share of a forward" figure.

    python tools/meshbench.py [--steps 200] [--repeats 5] [--forward] [--out profiles/mesh/meshbench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAL = dict(fx=3896.34, fy=3896.34, cx=1064.836, cy=976.456, baseline=173.557, doffs=163.863)       # Middlebury Bicycle2
MAX_JUMP = 1.0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh", "meshbench.txt"))
    a = ap.parse_args()
    import torch
    from s2m2_amd import hip
    from tools.kbench import captured, spread, timed
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
        for scene in ("piecewise", "constant"):
            g = torch.Generator(device="cuda").manual_seed(H + len(scene))
            if scene == "constant":
                disp = torch.full((1, 1, H, W), 100.0, device="cuda")
                conf = torch.ones((1, 1, H, W), device="cuda")
            else:
                # planes of 64 x 48 pixel blocks, gradients up to 0.3 px/px, 0.2 px of noise, block offsets of 0 .. 120 px
                v, u = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
                block = (v // 48) * 131 + (u // 64) * 37
                disp = (90.0 + (block % 25) * 5.0 + 0.3 * (u % 64) * ((block % 7) - 3) / 3.0 + 0.2 * (v % 48) * ((block % 5) - 2) / 2.0
                        + 0.2 * torch.rand((H, W), device="cuda", generator=g)).float()[None, None].contiguous()
                conf = (torch.rand((1, 1, H, W), device="cuda", generator=g) > 0.1).float()
            occ = torch.ones((1, 1, H, W), device="cuda")
            img = torch.randint(0, 256, (1, 3, H, W), device="cuda", dtype=torch.uint8, generator=g)
            records = torch.empty((1, H * W, 4), device="cuda", dtype=torch.int32)
            records15 = torch.empty((1, H * W, 4), device="cuda", dtype=torch.int32)
            faces = torch.empty((1, 2 * (H - 1) * (W - 1), 3), device="cuda", dtype=torch.int32)
            count, count15, fcount = (torch.zeros((1,), device="cuda", dtype=torch.int32) for _ in range(3))
            ws = torch.empty(hip.mesh_workspace_bytes(1, H, W), device="cuda", dtype=torch.uint8)
            ws15 = torch.empty(hip.cloud_workspace_bytes(1, H, W), device="cuda", dtype=torch.uint8)

            def k20():
                hip.mesh(disp, occ, conf, img, depth_trunc=3.0, max_jump=MAX_JUMP, records=records, count=count, faces=faces, face_count=fcount,
                         workspace=ws, **CAL)

            def k15():
                hip.cloud(disp, occ, conf, img, depth_trunc=3.0, records=records15, count=count15, workspace=ws15, **CAL)

            g20, g15 = captured(k20), captured(k15)
            bf, doffs = float(CAL["baseline"] * CAL["fx"]), CAL["doffs"]
            uu = torch.arange(W, device="cuda", dtype=torch.float32).expand(H, W)
            vv = torch.arange(H, device="cuda", dtype=torch.float32)[:, None].expand(H, W)

            def composed():
                D = disp[0, 0]
                valid = (conf[0, 0] > 0.1) & (occ[0, 0] > 0.5)
                d = torch.where(valid, D, -1.0)
                z = torch.where(d <= 0, 1e9, bf / (d + doffs)) / 1000.0
                keep = (z > 0) & (z < 3.0)
                flat = keep.reshape(-1)
                rank = torch.where(flat, torch.cumsum(flat, 0, dtype=torch.int32) - 1, -1).reshape(H, W)
                idx = torch.nonzero(flat).squeeze(1)                                        # synchronises
                zk = z.reshape(-1)[idx]
                x = (uu.reshape(-1)[idx] - CAL["cx"]) * zk / CAL["fx"]
                y = (vv.reshape(-1)[idx] - CAL["cy"]) * zk / CAL["fy"]
                verts, cols = torch.stack([x, y, zk], dim=1), img[0].reshape(3, -1)[:, idx].t().contiguous()
                ka, kb, kc, ke = keep[:-1, :-1], keep[:-1, 1:], keep[1:, :-1], keep[1:, 1:]
                da, db, dc, de = D[:-1, :-1], D[:-1, 1:], D[1:, :-1], D[1:, 1:]
                ra, rb, rc, re = rank[:-1, :-1], rank[:-1, 1:], rank[1:, :-1], rank[1:, 1:]
                j = lambda kp, kq, dp, dq: kp & kq & ((dp - dq).abs() <= MAX_JUMP)
                ac, ab, ce, be, ae, bc = j(ka, kc, da, dc), j(ka, kb, da, db), j(kc, ke, dc, de), j(kb, ke, db, de), j(ka, ke, da, de), j(kb, kc, db, dc)
                use_ae = torch.where(ka & kb & kc & ke, (da - de).abs() <= (db - dc).abs(), ~(kb & kc))
                f0 = torch.where(use_ae, ac & ce & ae, ac & bc & ab)
                f1 = torch.where(use_ae, ae & be & ab, bc & ce & be)
                t0 = torch.stack([ra, rc, torch.where(use_ae, re, rb)], dim=-1)
                t1 = torch.stack([torch.where(use_ae, ra, rb), torch.where(use_ae, re, rc), torch.where(use_ae, rb, re)], dim=-1)
                tri = torch.stack([t0, t1], dim=2).reshape(-1, 3)
                sel = torch.nonzero(torch.stack([f0, f1], dim=2).reshape(-1)).squeeze(1)    # synchronises
                return verts, cols, tri[sel]

            t20, t15, tt = [], [], []
            for _ in range(a.repeats):                               # alternated
                t20.append(timed(g20.replay, a.steps))
                t15.append(timed(g15.replay, a.steps))
                tt.append(timed(composed, max(20, a.steps // 4)))
            n, nf = int(count[0]), int(fcount[0])
            assert n == int(count15[0]) and torch.equal(records[0, :n], records15[0, :n])
            verts, _, tri = composed()
            # the composition is not the oracle (tests/test_hip_mesh.py is): torch evaluates the z chain in its own operation order, so a pixel
            # whose z rounds onto the truncation threshold may fall on the other side; where the vertex sets agree the faces must be equal
            assert abs(verts.shape[0] - n) <= 8, (verts.shape, n)
            if verts.shape[0] == n:
                assert torch.equal(tri, faces[0, :nf]), "the torch composition and K20 disagree"
            u20, u15, ut = statistics.median(t20), statistics.median(t15), statistics.median(tt)
            need15 = 15 * H * W + 16 * n
            need20 = need15 + 12 * nf
            say(f"{W}x{H} {scene}: kept {n / (H * W):.3f}, {nf / (H * W):.3f} faces per pixel")
            say(f"    K20 s2m2_mesh      {spread(t20)}   {need20 / 1e6:6.1f} MB mandatory = {need20 / u20 / 1e6:5.2f} TB/s = "
                f"{need20 / u20 / 1e6 / 8.0 * 100:4.1f} % of 8 TB/s"
                + (f"   {u20 / forward_us * 100:.2f} % of the S forward" if forward_us and H == 1024 else ""))
            say(f"    torch composition  {spread(tt)}   {ut / u20:5.1f}x K20")
            say(f"    K15 s2m2_cloud     {spread(t15)}   {need15 / 1e6:6.1f} MB mandatory = {need15 / u15 / 1e6:5.2f} TB/s = "
                f"{need15 / u15 / 1e6 / 8.0 * 100:4.1f} % of 8 TB/s   K20 / K15: {u20 / u15:4.2f}x the time, "
                f"{(need20 / u20) / (need15 / u15):4.2f}x the rate")
            del g20, g15

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
