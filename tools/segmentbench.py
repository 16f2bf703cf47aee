"""K22 (s2m2_segment: connected components + speckle filter, four launches) against its yardsticks, same box, same process, alternated: K15
(s2m2_cloud) and K20 (s2m2_mesh) alone on the same maps, K22 in front of K20 (the filtered map fed on), and the same labels composed from torch
ops -- min-label propagation over the joined edges with pointer jumping, looped until a sweep changes nothing.  That loop's sweep count depends
on the data and every sweep ends with a host synchronisation, which is why it cannot be captured; the count is printed: it is the point of the
comparison.

Shapes 1216x1024 and 2432x2048.  Scenes: `forward` (with --forward: the maps of an S forward of a synthetic pair at 1216x1024; at 2432x2048 the
same maps with every pixel doubled both ways), `one` (everything kept, one component), `singletons` (every pixel kept, noise disparity, max_jump
1: nearly every pixel its own component), `percolation` (site percolation at p = 0.593 with max_jump = inf: the tortuous worst case).

K22, K15, K20 and K22+K20 are timed with events around `--steps` replays of a hipGraph that holds one call; the torch loop is timed once with
events after one warm-up call.  Figures are the median of `--repeats` alternated windows with minimum and maximum.  Bytes: K22's MANDATORY
traffic -- the three maps read once (12 B per pixel) and the requested outputs written once (label 4, size 4, mask 1, disp_out 4 B per pixel)
-- over the measured time.

    python tools/segmentbench.py [--steps 200] [--repeats 5] [--forward] [--sizes 1024x1216,2048x2432] [--out profiles/segment/segmentbench.txt]
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAL = dict(fx=3896.34, fy=3896.34, cx=1064.836, cy=976.456, baseline=173.557, doffs=163.863)       # Middlebury Bicycle2
MIN_SIZE = 100


def torch_labels(torch, keep, disp, max_jump):
    """(H,W) bool, (H,W) fp32 -> (labels (H,W) int64 with H*W where not kept, sweeps): the propagation loop of tests/segment_oracle.py in torch"""
    H, W = keep.shape
    n = H * W
    jh = keep[:, :-1] & keep[:, 1:] & ((disp[:, :-1] - disp[:, 1:]).abs() <= max_jump)
    jv = keep[:-1, :] & keep[1:, :] & ((disp[:-1, :] - disp[1:, :]).abs() <= max_jump)
    big = torch.full((), n, device=keep.device, dtype=torch.int64)
    lab = torch.where(keep, torch.arange(n, device=keep.device).reshape(H, W), big)
    ext = torch.cat([lab.reshape(-1), big.reshape(1)])                  # slot n: the label of "not kept"
    sweeps = 0
    while True:
        lab = ext[:n].reshape(H, W)
        m = torch.where(jh, torch.minimum(lab[:, :-1], lab[:, 1:]), big)
        new = lab.clone()
        new[:, :-1] = torch.minimum(new[:, :-1], m)
        new[:, 1:] = torch.minimum(new[:, 1:], m)
        m = torch.where(jv, torch.minimum(new[:-1, :], new[1:, :]), big)
        new[:-1, :] = torch.minimum(new[:-1, :], m)
        new[1:, :] = torch.minimum(new[1:, :], m)
        nxt = torch.cat([new.reshape(-1), big.reshape(1)])
        for _ in range(3):                                               # pointer jumping, a fixed number of hops per sweep
            nxt = nxt[nxt]
        sweeps += 1
        if torch.equal(nxt, ext):                                        # synchronises
            return ext[:n].reshape(H, W), sweeps
        ext = nxt


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--sizes", default="1024x1216,2048x2432")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment", "segmentbench.txt"))
    a = ap.parse_args()
    import torch
    from s2m2_amd import hip
    from tools.kbench import captured, spread, timed
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    forward_us, fmaps = None, None
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
                fmaps = m(l, r)
            forward_us = statistics.median(timed(lambda: m(l, r), 50) for _ in range(a.repeats))
        fmaps = [t.float().contiguous().clone() for t in fmaps]
        say(f"S forward 1216x1024 fp16 (hipGraph replay, same session): {forward_us / 1000.0:.3f} ms")
        del m

    tr, tc = hip.segment_tile(1 << 12, 1 << 12)
    say(f"tile of the local pass: {tr} x {tc}; min_size {MIN_SIZE}; outputs: label, size, mask, disp_out, stats")
    for H, W in (tuple(int(x) for x in s.split("x")) for s in a.sizes.split(",")):
        for scene in (("forward",) if fmaps is not None else ()) + ("one", "singletons", "percolation"):
            g = torch.Generator(device="cuda").manual_seed(H + len(scene))
            one = torch.ones((1, 1, H, W), device="cuda")
            occ, conf, max_jump, cam = one, one, 1.0, dict(depth_trunc=3.0, **CAL)
            if scene == "forward":
                k = H // fmaps[0].shape[-2]
                disp, occ, conf = (t.repeat_interleave(k, -2).repeat_interleave(k, -1).contiguous() for t in fmaps)
                cam = dict(depth_trunc=1e9, **CAL)               # (a seeded model's disparities are small: no truncation)
            elif scene == "one":
                disp = torch.full((1, 1, H, W), 100.0, device="cuda")
            elif scene == "singletons":
                disp = (70.0 + 200.0 * torch.rand((1, 1, H, W), device="cuda", generator=g)).contiguous()
            else:
                disp = torch.full((1, 1, H, W), 100.0, device="cuda")
                conf = (torch.rand((1, 1, H, W), device="cuda", generator=g) < 0.593).float()
                max_jump = math.inf
            img = torch.randint(0, 256, (1, 3, H, W), device="cuda", dtype=torch.uint8, generator=g)
            label, size = (torch.empty((1, 1, H, W), device="cuda", dtype=torch.int32) for _ in range(2))
            mask = torch.empty((1, 1, H, W), device="cuda", dtype=torch.uint8)
            out = torch.empty((1, 1, H, W), device="cuda", dtype=torch.float32)
            stats = torch.zeros((1, 4), device="cuda", dtype=torch.int32)
            ws = torch.empty(hip.segment_workspace_bytes(1, H, W), device="cuda", dtype=torch.uint8)
            records = torch.empty((1, H * W, 4), device="cuda", dtype=torch.int32)
            faces = torch.empty((1, 2 * (H - 1) * (W - 1), 3), device="cuda", dtype=torch.int32)
            count, fcount = (torch.zeros((1,), device="cuda", dtype=torch.int32) for _ in range(2))
            ws20 = torch.empty(hip.mesh_workspace_bytes(1, H, W), device="cuda", dtype=torch.uint8)
            ws15 = torch.empty(hip.cloud_workspace_bytes(1, H, W), device="cuda", dtype=torch.uint8)

            def k22():
                hip.segment(disp, occ, conf, H=H, W=W, max_jump=max_jump, min_size=MIN_SIZE, workspace=ws, label=label, size=size, mask=mask,
                            disp_out=out, stats=stats, **cam)

            def k20(d=disp, unfiltered=False):
                hip.mesh(d, occ, conf, img, max_jump=max_jump, unfiltered=unfiltered, records=records, count=count, faces=faces, face_count=fcount,
                         workspace=ws20, **cam)

            def k15():
                hip.cloud(disp, occ, conf, img, records=records, count=count, workspace=ws15, **cam)

            def k22_k20():
                k22()
                k20(out, True)

            graphs = [captured(f) for f in (k22, k15, k20, k22_k20)]
            ts = [[] for _ in graphs]
            for _ in range(a.repeats):                               # alternated
                for t, gr in zip(ts, graphs):
                    t.append(timed(gr.replay, a.steps))
            graphs[0].replay()
            torch.cuda.synchronize()
            st = stats[0].tolist()

            bf = float(CAL["baseline"] * CAL["fx"])

            def composed():
                D = disp[0, 0]
                valid = (conf[0, 0] > 0.1) & (occ[0, 0] > 0.5)
                d = torch.where(valid, D, -1.0)
                z = torch.where(d <= 0, 1e9, bf / (d + CAL["doffs"])) / 1000.0
                keep = (z > 0) & (z < cam["depth_trunc"])
                return keep, *torch_labels(torch, keep, D, max_jump)

            keep, lab, sweeps = composed()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            composed()
            t1.record()
            torch.cuda.synchronize()
            ut = 1000.0 * t0.elapsed_time(t1)
            # the composition is not the oracle (tests/test_hip_segment.py is): torch evaluates the z chain in its own operation order, so a
            # pixel on the truncation threshold may fall on the other side; where the kept sets agree the labels must be equal
            same_keep = torch.equal(keep, label[0, 0] >= 0)
            if same_keep:
                assert torch.equal(torch.where(keep, lab, -1).int(), label[0, 0]), "the torch composition and K22 disagree"
            u22, u15, u20, u2220 = (statistics.median(t) for t in ts)
            need = (12 + 4 + 4 + 1 + 4) * H * W
            border = (W - 1) // tc * H + (H - 1) // tr * W
            say(f"{W}x{H} {scene}: kept {st[0]}, components {st[1]}, surviving {st[2]} in {st[3]} components"
                + ("" if same_keep else "   (torch keeps another pixel set: labels not compared)"))
            say(f"    K22 s2m2_segment   {spread(ts[0])}   4 launches, {border} border threads   {need / 1e6:6.1f} MB mandatory = "
                f"{need / u22 / 1e6:5.2f} TB/s" + (f"   {u22 / forward_us * 100:.2f} % of the S forward" if forward_us and H == 1024 else ""))
            say(f"    torch propagation  {ut:8.1f} us   {sweeps} sweeps   {ut / u22:6.1f}x K22")
            say(f"    K15 s2m2_cloud     {spread(ts[1])}   K22 / K15: {u22 / u15:4.2f}x")
            say(f"    K20 s2m2_mesh      {spread(ts[2])}   K22 / K20: {u22 / u20:4.2f}x")
            say(f"    K22 + K20          {spread(ts[3])}   over K20 alone: {u2220 - u20:+.1f} us")
            del graphs

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
