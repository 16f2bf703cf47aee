"""Engine file vs S2M2.forward at one configuration (default: S 1216x1024 fp16, B = 1, the bench configuration): ms per pair of the stand-alone
runner (s2m2_run_engine --repeat, a fresh process per measurement) against the forward's hipGraph replay in this process, alternated, a few
repeats each; the engine file's size.  One JSON line.

    python tools/engine_bench.py [--model S] [--height 1024] [--width 1216] [--steps 200] [--repeats 4]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="S")
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=4)
    a = ap.parse_args()
    import torch
    from s2m2_amd.build import RUNNER
    from s2m2_amd.export import export_engine
    from s2m2_amd.model import build_model
    from s2m2_amd.spec import MODEL_CONFIGS
    from s2m2_amd.weights import seeded_state_dict, synthetic_pair
    C, ntr = MODEL_CONFIGS[a.model]
    m = build_model(a.model)
    m.load_state_dict(seeded_state_dict(C, 1, ntr, 0), strict=True)
    m = m.cuda().eval()
    H, W = a.height, a.width
    l, r = synthetic_pair(H, W, 1, 32, 0)
    l, r = l.cuda().contiguous(), r.cuda().contiguous()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "engine.s2m2")
        info = export_engine(m, path, H, W)
        for name, t in (("left.f32", l), ("right.f32", r)):
            t.cpu().numpy().astype("<f4").tofile(os.path.join(tmp, name))

        def engine_ms() -> float:
            p = subprocess.run([RUNNER, path, os.path.join(tmp, "left.f32"), os.path.join(tmp, "right.f32"), "--repeat", str(a.steps)],
                               capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                raise RuntimeError(p.stderr)
            return json.loads(p.stdout.strip().splitlines()[-1])["ms_per_pair"]

        def forward_ms() -> float:
            with torch.autocast("cuda", dtype=torch.float16):
                for _ in range(3):                                 # eager, capture, replay
                    m(l, r)
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.steps):
                    m(l, r)
                t1.record()
                t1.synchronize()
            return t0.elapsed_time(t1) / a.steps

        eng, fwd = [], []
        for _ in range(a.repeats):
            eng.append(engine_ms())
            fwd.append(forward_ms())
    res = {"config": f"{a.model} {W}x{H} fp16 B=1", "steps": a.steps, "engine_ms": eng, "forward_ms": fwd,
           "engine_median": statistics.median(eng), "forward_median": statistics.median(fwd),
           "engine_spread": max(eng) - min(eng), "forward_spread": max(fwd) - min(fwd),
           "engine_file_bytes": info["bytes"], "launches": info["launches"]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
