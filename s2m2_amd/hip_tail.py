"""K19 (``s2m2_conv_block_tail``, csrc/convtail.hip): the second half of a ConvBlock2D per launch.  The descriptor mirror and the signature are in
hip.py with all the others (``hip.load()`` binds every symbol there); this module holds the wrapper, which hip.py re-exports as
``hip.conv_block_tail``."""
import ctypes
from typing import Optional, Tuple

import torch

from . import hip as _h


def conv_block_tail_supported(C: int, H: int, W: int, dtype: torch.dtype) -> bool:
    """K19 (conv_block_tail) takes the second half of a ConvBlock2D of this width on an H x W grid (fp16, C = 128 / 256)"""
    return bool(_h.load().s2m2_conv_block_tail_supported(C, H, W, _h._DT[dtype]))


def conv_block_tail(t: torch.Tensor, z: torch.Tensor, w_conv2: torch.Tensor, b_conv2, w_1x0: torch.Tensor, b_1x0, w_1x2: torch.Tensor, b_1x2,
                    out: Optional[torch.Tensor] = None, patch: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """K19: convs.2(t) + convs_1x.2(ReLU(convs_1x.0(z))) of a ConvBlock2D (attentions.py:255-281) on t = GELU(convs.0(z)) and z (N,H,W,C) in one
    launch, bit-identical to mlp_chain(z, [ReLU stage, plain stage], frag=True) followed by conv2d(t, ..., epi=EPI_ADD, aux0=b, korder=2).
    w_conv2: the 3x3 layer as a K5 v5 fragment stream (pack.pack_conv_frag), w_1x0 / w_1x2: the 1x1 layers in K9's fragment order
    (pack.chain_frag); biases fp32 (C) or None.  out: an (N,H,W,C) fp16 view to write (pixel stride a multiple of 8), else a new tensor;
    patch: (2, 32), (4, 32) or (4, 40) forces the block's pixel patch."""
    _h._resident("conv_block_tail", t, z, w_conv2, b_conv2, w_1x0, b_1x0, w_1x2, b_1x2, out)
    if t.dtype != torch.float16 or z.dtype != torch.float16 or tuple(t.shape) != tuple(z.shape):
        raise ValueError("conv_block_tail: t and z must be (N,H,W,C) fp16 tensors of one shape")
    ts, zs = _h._pixels(t, "conv_block_tail: t"), _h._pixels(z, "conv_block_tail: z")
    N, H, W, C = t.shape
    if out is None:
        out = torch.empty((N, H, W, C), device=t.device, dtype=t.dtype)
    elif out.dtype != t.dtype or tuple(out.shape) != tuple(t.shape):
        raise ValueError("conv_block_tail: out must be an fp16 tensor of t's shape")
    os_ = _h._pixels(out, "conv_block_tail: out")
    _h._vec(w_conv2, 9 * C * C, "conv_block_tail: w_conv2", dtype=t.dtype)
    _h._vec(w_1x0, C * C, "conv_block_tail: w_1x0", dtype=t.dtype)
    _h._vec(w_1x2, C * C, "conv_block_tail: w_1x2", dtype=t.dtype)
    for name, b in (("b_conv2", b_conv2), ("b_1x0", b_1x0), ("b_1x2", b_1x2)):
        _h._vec(b, C, f"conv_block_tail: {name}", optional=True)
    d = _h.ConvTailDesc()
    d.t, d.t_stride, d.z, d.z_stride, d.out, d.out_stride = t.data_ptr(), ts, z.data_ptr(), zs, out.data_ptr(), os_
    d.N, d.H, d.W, d.C = N, H, W, C
    d.w_conv2, d.w_1x0, d.w_1x2 = w_conv2.data_ptr(), w_1x0.data_ptr(), w_1x2.data_ptr()
    d.b_conv2, d.b_1x0, d.b_1x2 = _h._ptr(b_conv2), _h._ptr(b_1x0), _h._ptr(b_1x2)
    d.patch_rows, d.patch_cols = patch if patch is not None else (0, 0)
    d.dtype = _h._DT[t.dtype]
    _h._check(_h.load().s2m2_conv_block_tail(ctypes.byref(d), _h._stream()), "s2m2_conv_block_tail")
    _h._meter("conv_block_tail", 2.0 * N * H * W * C * C * 11)
    return out
