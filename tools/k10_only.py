#!/usr/bin/env python3
"""The direct K10 form alone at the forward's 1/4-level shapes (z1 read through the x2 resampling), a few launches each: the target of a
counter pass (rocprofv3 --pmc ... -- python tools/k10_only.py) or of a kernel trace, without the rest of the forward around it.

    python tools/k10_only.py [launches=6]
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from s2m2_amd import hip, pack  # noqa: E402

# (n, h, w, C) of z0; z1 is the (n, h/2, w/2, C) tensor
SHAPES = [(2, 256, 304, 128), (1, 256, 304, 128), (2, 128, 152, 128), (2, 64, 76, 256)]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    for n, h, w, C in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        z0 = torch.randn(n, h, w, C, device="cuda", generator=g).half()
        z1 = torch.randn(n, h // 2, w // 2, C, device="cuda", generator=g).half()
        w1 = pack.pack_conv((torch.randn(3 * C, 2 * C, 1, 1, device="cuda", generator=g) / math.sqrt(2 * C)).half(), torch.float16)
        w2 = pack.pack_conv((torch.randn(C, 3 * C, 1, 1, device="cuda", generator=g) / math.sqrt(2 * C)).half(), torch.float16)
        b1, bg, bf = (torch.randn(k, device="cuda", generator=g) for k in (3 * C, C, C))
        ws = pack.fusion_frag(w1, w2)
        for _ in range(reps):
            y = hip.feature_fusion(z0, z1, ws, b1, None, bg, bf, z1_coarse=True, frag=True)
        torch.cuda.synchronize()
        print(f"rows {n * h * w:7d} C {C}: {reps} launches, checksum {float(y.float().abs().mean()):.6f}", flush=True)


if __name__ == "__main__":
    main()
