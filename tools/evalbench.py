"""K18 (s2m2_disp_eval: disparity error statistics against ground truth, two launches) against the same statistics composed from torch ops on the
device tensors -- masks, where, round, sums, index_add for the histogram and the confidence table: what a user writes without K18 and without
leaving the GPU -- at 1216x1024 and 2432x2048, with and without occ / conf.  Same box, same process, alternated, a few repeats each (medians).

K18 is timed with events around `--steps` replays of a hipGraph that holds one call; the torch composition with events around eager calls (it
has no synchronising op, so the events bracket device work only).  Bytes: the algorithmic bytes of DESIGN.md (K18) -- every input read once,
21 B per pixel with occ / conf / region, 9 B without occ / conf; the partial blocks and the stat block are not counted -- over the time,
as a share of 8 TB/s.  With --forward the S forward (fp16, hipGraph replay) is timed in the same session at 1216x1024 for the "share of a
forward" line.  The composition is checked against K18's words before it is timed (it is not the oracle: tests/test_hip_eval.py is).

    python tools/evalbench.py [--steps 1000] [--repeats 5] [--forward] [--out profiles/eval/evalbench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THR = (0.5, 1.0, 2.0, 4.0)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval", "evalbench.txt"))
    a = ap.parse_args()
    import torch
    from s2m2_amd import hip
    from tools.kbench import captured, timed
    if not torch.cuda.is_available():
        raise SystemExit("evalbench: needs the GPU (nothing is measured without one)")
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
        g = torch.Generator(device="cuda").manual_seed(H)
        disp = torch.rand((1, 1, H, W), device="cuda", generator=g) * 320.0 - 20.0
        conf = torch.rand((1, 1, H, W), device="cuda", generator=g)
        occ = torch.rand((1, 1, H, W), device="cuda", generator=g)
        scale = 10.0 ** (torch.rand((1, 1, H, W), device="cuda", generator=g) * 3.0 - 2.0)
        gt = disp + scale * (torch.rand((1, 1, H, W), device="cuda", generator=g) - 0.5).sign()
        gt[torch.rand((1, 1, H, W), device="cuda", generator=g) < 0.1] = float("inf")
        region = (torch.rand((1, 1, H, W), device="cuda", generator=g) >= 0.2).to(torch.uint8)
        for with_conf in (True, False):
            stats = torch.zeros((1, hip.EVAL_WORDS), device="cuda", dtype=torch.int64)
            ws = torch.empty(hip.eval_workspace_bytes(1, H, W), device="cuda", dtype=torch.uint8)
            kw = dict(region=region, occ=occ if with_conf else None, conf=conf if with_conf else None, thresholds=THR)

            def k18():
                hip.disp_eval(disp, gt, stats, ws, **kw)

            graph = captured(k18)

            def block(sel, a_, q, s, finite, bad, d1):
                """the 14 words of one set of pixels (sel: evaluated pixels of the set)"""
                summed = sel & finite
                return torch.stack([sel.sum(), (sel & ~finite).sum(), (q * summed).sum(), (s * summed).sum(), (sel & d1).sum()]
                                   + [(sel & b).sum() for b in bad])

            def composed():
                d, t = disp.reshape(-1), gt.reshape(-1)
                ev = (region.reshape(-1) != 0) & torch.isfinite(t) & (t > 0.0)
                e = d - t
                a_ = e.abs()
                finite = torch.isfinite(d)
                q = torch.round(a_.clamp(max=1024.0) * 65536.0).to(torch.int64)
                s = torch.round((e * e).clamp(max=1048576.0) * 4096.0).to(torch.int64)
                bad = [~finite | (a_ > th) for th in THR]
                d1 = ~finite | ((a_ > 3.0) & (a_ > 0.05 * t.abs()))
                out = [block(ev, a_, q, s, finite, bad, d1)]
                summed = ev & finite
                hbin = torch.nan_to_num(a_ * 64.0, nan=1024.0).clamp(max=1024.0).floor().to(torch.int64)
                out.append(torch.zeros(hip.EVAL_HIST_BINS, device="cuda", dtype=torch.int64).index_add_(0, hbin, summed.to(torch.int64)))
                if with_conf:
                    c, o = conf.reshape(-1), occ.reshape(-1)
                    out.append(block(ev & (c > 0.1) & (o > 0.5), a_, q, s, finite, bad, d1))
                    cbin = torch.nan_to_num(c * 64.0, nan=0.0).floor().clamp(0, 63).to(torch.int64)
                    cols = torch.stack([ev.to(torch.int64), q * summed] + [(ev & b).to(torch.int64) for b in bad], dim=1)
                    out.append(torch.zeros((hip.EVAL_CONF_BINS, cols.shape[1]), device="cuda", dtype=torch.int64).index_add_(0, cbin, cols))
                return out

            # the composition computes what K18 computes (fp32 chain in the same order; it is checked, not asserted to be the oracle)
            graph.replay()
            torch.cuda.synchronize()
            w = stats[0]
            got = composed()
            pick = [hip.EVAL_N_EVAL, hip.EVAL_N_NONFINITE, hip.EVAL_SUM_ABS_Q, hip.EVAL_SUM_SQ_Q, hip.EVAL_D1_BAD] + [hip.EVAL_BAD + i for i in range(len(THR))]
            agree = torch.equal(got[0], w[pick]) and torch.equal(got[1], w[hip.EVAL_HIST:hip.EVAL_CONF])
            if with_conf:
                table = w[hip.EVAL_CONF:].reshape(hip.EVAL_CONF_BINS, hip.EVAL_CONF_ROW_WORDS)[:, :2 + len(THR)]
                agree = agree and torch.equal(got[2], w[[hip.EVAL_KEPT + i for i in pick]]) and torch.equal(got[3], table)

            t_k18, t_torch = [], []
            for _ in range(a.repeats):                               # alternated
                t_k18.append(timed(graph.replay, a.steps))
                t_torch.append(timed(composed, max(10, a.steps // 20)))
            us, ut = statistics.median(t_k18), statistics.median(t_torch)
            moved = (21 if with_conf else 9) * H * W
            say(f"{W}x{H} {'with occ/conf' if with_conf else 'disp only    '}: K18 {us:8.1f} us (min {min(t_k18):.1f} max {max(t_k18):.1f})   "
                f"torch composition {ut:9.1f} us   ratio {ut / us:6.1f}x   composition agrees: {'yes' if agree else 'NO'}   "
                f"{moved / 1e6:6.1f} MB algorithmic = {moved / us / 1e6:6.3f} TB/s = {moved / us / 1e6 / 8.0 * 100:4.1f} % of 8 TB/s"
                + (f"   {us / forward_us * 100:.2f} % of the S forward" if forward_us and H == 1024 else ""))
            del graph

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
