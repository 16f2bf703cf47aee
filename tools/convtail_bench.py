#!/usr/bin/env python3
"""K19 (s2m2_conv_block_tail: the second half of a ConvBlock2D in one launch) against the launches it replaces, on the grids of the S model above
K14's (fp16, hipGraph replay): the three-launch block (K9 chain, convs.0, convs.2 + residual) against convs.0 + K19, per patch form, and K14
for information where it exists.  The two paths alternate, three rounds each; the line gives every round."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from s2m2_amd import hip, pack  # noqa: E402
from tools.kbench import timeit_graph  # noqa: E402

SHAPES = [(1, 256, 304, 128), (2, 256, 304, 128), (1, 64, 76, 256), (2, 64, 76, 256), (1, 128, 152, 128)]
F16 = torch.float16
for N, H, W, C in SHAPES:
    g = torch.Generator(device="cuda").manual_seed(0)
    k0 = (torch.randn(C, C, 3, 3, device="cuda", generator=g) / math.sqrt(9 * C)).half()
    k2 = (torch.randn(C, C, 3, 3, device="cuda", generator=g) / math.sqrt(9 * C)).half()
    p0 = (torch.randn(C, C, 1, 1, device="cuda", generator=g) / math.sqrt(C)).half()
    p2 = (torch.randn(C, C, 1, 1, device="cuda", generator=g) / math.sqrt(C)).half()
    bs = [torch.randn(C, device="cuda") * 0.3 for _ in range(4)]
    x = torch.randn(N, H, W, C, device="cuda", generator=g).half()
    w0, w2 = pack.pack_conv_frag(k0, F16), pack.pack_conv_frag(k2, F16)
    a0, a2 = pack.chain_frag(pack.pack_conv(p0, F16)), pack.chain_frag(pack.pack_conv(p2, F16))

    def triple():
        b = hip.mlp_chain(x, [(a0, bs[2], hip.ACT_RELU, None), (a2, bs[3], hip.ACT_NONE, None)], frag=True)
        t = hip.conv2d([x], w0, bs[0], 3, 3, C, act=hip.ACT_GELU, korder=2)
        return hip.conv2d([t], w2, bs[1], 3, 3, C, epi=hip.EPI_ADD, aux0=b, korder=2)

    def tail(patch=None):
        t = hip.conv2d([x], w0, bs[0], 3, 3, C, act=hip.ACT_GELU, korder=2)
        return hip.conv_block_tail(t, x, w2, bs[1], a0, bs[2], a2, bs[3], patch=patch)

    assert torch.equal(triple(), tail())
    old, new = [], []
    for _ in range(3):
        old.append(timeit_graph(triple, 20, 3))
        new.append(timeit_graph(tail, 20, 3))
    fmt = lambda v: " / ".join(f"{t:.1f}" for t in v)         # noqa: E731
    line = f"({N},{H},{W},{C}): chain + conv + conv {fmt(old)} us   conv + conv_block_tail {fmt(new)} us   ({min(new) - min(old):+.1f} us)"
    for patch in ((2, 32), (4, 32), (4, 40)):
        line += f"   {patch[0]}x{patch[1]} {timeit_graph(lambda: tail(patch), 20, 3):.1f}"
    if hip.conv_block_supported(C, H, W, F16):
        line += f"   K14 {timeit_graph(lambda: hip.conv_block(x, w0, bs[0], w2, bs[1], a0, bs[2], a2, bs[3]), 20, 3):.1f}"
    print(line, flush=True)
