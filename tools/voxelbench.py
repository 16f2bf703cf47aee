"""K23 (s2m2_voxel: voxel-grid downsampling of the point cloud) against its yardsticks, same box, same process, alternated: the same records
composed from torch ops (keys, ``torch.unique(return_inverse=True)``, ``index_add_``, the ordering by first index -- several passes, a sort
and a host synchronisation to size the result), K15 (s2m2_cloud) alone on the same maps, and the build WITHOUT run combining
(``S2M2_LIB_SUFFIX=_voxel_plain S2M2_BUILD_DEFINES=-DS2M2_VOXEL_COMBINE=0 python -m s2m2_amd.build``; skipped where that library is absent).

Shapes 1216x1024 and 2432x2048.  Scene: a slanted plane near 2 m with a quarter pixel of disparity noise under the Bicycle2 camera, everything kept
(`all`) or a tenth of the pixels dropped at random (`tenth`); the voxel sizes are searched on the scene (bisection on K23's own stats) so that
a voxel holds about 4, 30 and 300 pixels.  With --forward also the maps of an S forward of a synthetic pair (1216x1024; doubled at 2432x2048).

K23, K15 and the plain build are timed with events around `--steps` replays of a hipGraph that holds one call; the torch composition, which
synchronises with the host and cannot be captured, with events around three eager calls after a warm-up call, in the same alternated windows.
Figures are the median of `--repeats` alternated windows with minimum and maximum.

Two derived numbers.  ATOMICS: an insertion issues 64 bytes of atomic payload (an 8-byte compare-and-swap or key load, two 4-byte and six
8-byte operations); the plain build inserts once per point in range, the shipped build at least once per run of equal consecutive voxels of
a row (counted from the index map; runs are cut further at wave borders, so this is a lower bound).  Payload over the time of ALL of K23's
launches is a lower bound of the rate the insert launch reaches; it is printed next to the two figures of the microarchitecture guide for
global fp32 atomic adds, about 1.3 TB/s for contiguous 256-byte wave instructions and 0.08 TB/s with 64 lanes in 64 unrelated lines --
integer atomics are not measured there, and nothing here measures the probe-length distribution: both are open.  TABLE ROOM: K23 with a table twice as large, which shows what a nearly full table costs.

The launches one by one (the clear launch's share) are not timed here: `--launches H W MILLIMETRES` only runs K23 `--steps` times on the `all`
scene at that voxel size, for a kernel trace of its own around it (rocprofv3 --kernel-trace --stats -- python tools/voxelbench.py --launches ...;
the per-kernel averages are filed as profiles/voxel/launches.txt).

    python tools/voxelbench.py [--steps 100] [--repeats 5] [--forward] [--sizes 1024x1216,2048x2432] [--out profiles/voxel/voxelbench.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAL = dict(fx=3896.34, fy=3896.34, cx=1064.836, cy=976.456, baseline=173.557, doffs=163.863)       # Middlebury Bicycle2
INSERT_BYTES = 64


def torch_voxels(torch, disp, occ, conf, img, vs, trunc):
    """the records of K23 composed from torch ops -> (xyz (n,3) fp32, rgb (n,3) uint8, weights (n) int64), in the order of first"""
    D = disp[0, 0]
    H, W = D.shape
    valid = (conf[0, 0] > 0.1) & (occ[0, 0] > 0.5)
    d = torch.where(valid, D, -1.0)
    z = torch.where(d <= 0, 1e9, float(CAL["baseline"] * CAL["fx"]) / (d + CAL["doffs"])) / 1000.0
    keep = (z > 0) & (z < trunc)
    v, u = torch.meshgrid(torch.arange(H, device=D.device, dtype=torch.float32), torch.arange(W, device=D.device, dtype=torch.float32), indexing="ij")
    q = torch.tensor(vs, dtype=torch.float32) / 1024.0
    q = float(q)
    X = torch.round(((u - CAL["cx"]) * z / CAL["fx"]) / q)
    Y = torch.round(((v - CAL["cy"]) * z / CAL["fy"]) / q)
    Z = torch.round(z / q)
    ok = keep & (X.abs() < 2.0 ** 30) & (Y.abs() < 2.0 ** 30) & (Z.abs() < 2.0 ** 30)
    pix = torch.nonzero(ok.reshape(-1)).reshape(-1)                                  # synchronises
    Q = torch.stack([X.reshape(-1)[pix], Y.reshape(-1)[pix], Z.reshape(-1)[pix]], 1).long()
    cell, local = Q >> 10, Q & 1023
    keys = ((cell[:, 0] + (1 << 20)) << 42) | ((cell[:, 1] + (1 << 20)) << 21) | (cell[:, 2] + (1 << 20))
    uniq, inv = torch.unique(keys, return_inverse=True)                              # sorts; synchronises
    nv = uniq.numel()
    n = torch.zeros(nv, dtype=torch.int64, device=D.device).index_add_(0, inv, torch.ones_like(inv))
    sums = torch.zeros((nv, 3), dtype=torch.int64, device=D.device).index_add_(0, inv, local)
    csum = torch.zeros((nv, 3), dtype=torch.int64, device=D.device).index_add_(0, inv, img[0].reshape(3, -1)[:, pix].T.long())
    first = torch.full((nv,), H * W, dtype=torch.int64, device=D.device).scatter_reduce_(0, inv, pix, "amin")
    order = torch.argsort(first)
    cells = torch.zeros((nv, 3), dtype=torch.int64, device=D.device)
    cells[inv] = cell                                                                # every writer of a row writes the same cell
    centre = ((cells.double() * 1024.0 + sums.double() / n.double()[:, None]) * q).float()
    colour = ((2 * csum + n[:, None]) // (2 * n[:, None])).to(torch.uint8)
    return centre[order], colour[order], n[order]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--sizes", default="1024x1216,2048x2432")
    ap.add_argument("--launches", nargs=3, metavar=("H", "W", "MILLIMETRES"), help="only run K23 on the `all` scene at this voxel size (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel", "voxelbench.txt"))
    a = ap.parse_args()
    import torch
    from s2m2_amd import hip
    from tools.kbench import captured, spread, timed
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    if a.launches:
        H, W, vs = int(a.launches[0]), int(a.launches[1]), float(a.launches[2]) / 1000.0
        g = torch.Generator(device="cuda").manual_seed(H)
        one = torch.ones((1, 1, H, W), device="cuda")
        img = torch.randint(0, 256, (1, 3, H, W), device="cuda", dtype=torch.uint8, generator=g)
        vv, uu = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
        plane = (170.0 + 0.02 * uu + 0.01 * vv + 0.25 * torch.rand((H, W), device="cuda", generator=g))[None, None].contiguous()
        mv = H * W // 4
        out = dict(records=torch.empty((1, mv, 4), device="cuda", dtype=torch.int32), weights=torch.empty((1, mv), device="cuda", dtype=torch.int32),
                   count=torch.zeros((1,), device="cuda", dtype=torch.int32), stats=torch.zeros((1, 4), device="cuda", dtype=torch.int32))
        ws = torch.empty(hip.voxel_workspace_bytes(1, H, W, mv), device="cuda", dtype=torch.uint8)
        for _ in range(a.steps):
            hip.voxel(plane, one, one, img, voxel_size=vs, max_voxels=mv, workspace=ws, depth_trunc=50.0, **out, **CAL)
        torch.cuda.synchronize()
        st = out["stats"][0].tolist()
        print(f"{W}x{H} all voxel {vs * 1000:.2f} mm: {a.steps} calls, max_voxels {mv}, stats {st}: {(st[0] - st[1]) / max(st[3], 1):.1f} points per voxel")
        return

    shipped = hip.load()
    plain = None
    plain_path = hip.LIB_PATH.replace(".so", "_voxel_plain.so")
    if os.path.exists(plain_path):
        plain = ctypes.CDLL(plain_path)
        for name, (res, args) in hip.SIGNATURES.items():
            fn = getattr(plain, name)
            fn.restype, fn.argtypes = res, args
    say("build without run combining: " + ("present (A/B below, alternated in this process)" if plain else "ABSENT (no A/B in this run)"))

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

    for H, W in (tuple(int(x) for x in s.split("x")) for s in a.sizes.split(",")):
        g = torch.Generator(device="cuda").manual_seed(H)
        one = torch.ones((1, 1, H, W), device="cuda")
        img = torch.randint(0, 256, (1, 3, H, W), device="cuda", dtype=torch.uint8, generator=g)
        vv, uu = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
        plane = (170.0 + 0.02 * uu + 0.01 * vv + 0.25 * torch.rand((H, W), device="cuda", generator=g))[None, None].contiguous()
        tenth = (torch.rand((1, 1, H, W), device="cuda", generator=g) >= 0.1).float()
        scenes = [("all", plane, one, one, 50.0), ("tenth", plane, one, tenth, 50.0)]
        if fmaps is not None:
            k = H // fmaps[0].shape[-2]
            scenes.append(("forward",) + tuple(t.repeat_interleave(k, -2).repeat_interleave(k, -1).contiguous() for t in fmaps) + (50.0,))
        mv = H * W // 4
        records = torch.empty((1, H * W, 4), device="cuda", dtype=torch.int32)
        weights = torch.empty((1, H * W), device="cuda", dtype=torch.int32)
        index = torch.empty((1, 1, H, W), device="cuda", dtype=torch.int32)
        count = torch.zeros((1,), device="cuda", dtype=torch.int32)
        stats = torch.zeros((1, 4), device="cuda", dtype=torch.int32)
        ws15 = torch.empty(hip.cloud_workspace_bytes(1, H, W), device="cuda", dtype=torch.uint8)
        say(f"{W}x{H}: max_voxels {mv} ({hip.voxel_slots(mv)} slots, {hip.voxel_workspace_bytes(1, H, W, mv) / 2 ** 20:.0f} MiB workspace)")
        for scene, disp, occ, conf, trunc in scenes:
            cam = dict(depth_trunc=trunc, **CAL)

            def k23(vs, max_voxels=mv, want_index=False):
                ws = k23.ws.setdefault(max_voxels, torch.empty(hip.voxel_workspace_bytes(1, H, W, max_voxels), device="cuda", dtype=torch.uint8))
                hip.voxel(disp, occ, conf, img, voxel_size=vs, max_voxels=max_voxels, workspace=ws, records=records, weights=weights, count=count,
                          index=index if want_index else None, stats=stats, **cam)
            k23.ws = {}

            def ratio(vs):
                k23(vs, max_voxels=H * W)
                torch.cuda.synchronize()
                st = stats[0].tolist()
                return (st[0] - st[1]) / max(st[3], 1)

            for target in (4, 30, 300):
                lo, hi = 1e-4, 1.0                                   # pixels per voxel grow with the size: bisection in the logarithm
                for _ in range(18):
                    mid = (lo * hi) ** 0.5
                    lo, hi = (mid, hi) if ratio(mid) < target else (lo, mid)
                vs = round(hi, 5)
                mvr = mv
                k23(vs, want_index=True)
                torch.cuda.synchronize()
                st = stats[0].tolist()
                if st[2]:                                            # more voxels than the default table takes: this row runs with twice the room
                    mvr = 2 * mv
                    k23(vs, max_voxels=mvr, want_index=True)
                    torch.cuda.synchronize()
                    st = stats[0].tolist()
                    say(f"  {scene} voxel {vs * 1000:.2f} mm: more than the default max_voxels: this row with max_voxels {mvr}")
                idx = index[0, 0]
                runs = int(((idx[:, 1:] != idx[:, :-1]) & (idx[:, 1:] >= 0)).sum() + (idx[:, 0] >= 0).sum())
                points = st[0] - st[1]

                def k15():
                    hip.cloud(disp, occ, conf, img, records=records, count=count, workspace=ws15, **cam)

                def with_lib(lib, f):
                    hip._lib = lib
                    try:
                        return captured(f)
                    finally:
                        hip._lib = shipped

                graphs = [captured(lambda: k23(vs, max_voxels=mvr)), captured(k15), captured(lambda: k23(vs, max_voxels=2 * mvr)),
                          captured(lambda: k23(vs, max_voxels=mvr, want_index=True))]
                if plain:
                    graphs.append(with_lib(plain, lambda: k23(vs, max_voxels=mvr)))
                ts, tt = [[] for _ in graphs], []
                for _ in range(a.repeats):                           # alternated
                    for t, gr in zip(ts, graphs):
                        t.append(timed(gr.replay, a.steps))
                    tt.append(timed(lambda: torch_voxels(torch, disp, occ, conf, img, vs, trunc), 3))
                u23, u15, u23x2, u23i = (statistics.median(t) for t in ts[:4])
                ut = statistics.median(tt)
                xyz, rgb, wt = torch_voxels(torch, disp, occ, conf, img, vs, trunc)
                graphs[0].replay()
                torch.cuda.synchronize()
                nv = int(count[0])
                # the composition is not the oracle (tests/test_hip_voxel.py is): torch evaluates the z chain in its own operation order
                same = xyz.shape[0] == nv and torch.equal(wt.int(), weights[0, :nv]) and torch.equal(xyz.view(torch.int32), records[0, :nv, :3])
                say(f"  {scene} voxel {vs * 1000:.2f} mm: {points} points in {nv} voxels ({points / max(nv, 1):.1f} per voxel), {runs} row runs"
                    f" ({points / max(runs, 1):.1f} points per run); torch composition " + ("bit-equal" if same else "NOT bit-equal (its own operation order)"))
                say(f"    K23 s2m2_voxel     {spread(ts[0])}   4 launches" +
                    (f"   {u23 / forward_us * 100:.2f} % of the S forward" if forward_us and H == 1024 else ""))
                say(f"    K23 with index     {spread(ts[3])}   5 launches")
                say(f"    torch composition  {spread(tt)}   {ut / u23:6.1f}x K23")
                say(f"    K15 s2m2_cloud     {spread(ts[1])}   K23 / K15: {u23 / u15:4.2f}x")
                say(f"    K23, 2x max_voxels {spread(ts[2])}   {u23x2 / u23:4.2f}x K23")
                say(f"    atomics, shipped   >= {runs * INSERT_BYTES / u23 / 1e6:6.3f} TB/s over all of K23 ({runs} insertions at least)")
                if plain:
                    up = statistics.median(ts[4])
                    say(f"    K23 plain build    {spread(ts[4])}   plain / shipped: {up / u23:4.2f}x   atomics {points * INSERT_BYTES / up / 1e6:6.3f} TB/s over all of K23"
                        f"   (fp32 adds: 1.3 TB/s contiguous, 0.08 TB/s scattered)")
                del graphs

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
