"""K17 (``s2m2_conv_gru``, csrc/convgru.hip): one ConvGRU half per launch.  The descriptor mirror and the signature are in hip.py with all the
others (``hip.load()`` binds every symbol there); this module holds the wrapper, which hip.py re-exports as ``hip.conv_gru``."""
import ctypes

import torch

from . import hip as _h


def conv_gru_supported(C: int, H: int, W: int, dtype: torch.dtype) -> bool:
    """K17 (conv_gru) takes a ConvGRU half of this width on an H x W grid (fp16, hidden and input width 128)"""
    return bool(_h.load().s2m2_conv_gru_supported(C, H, W, _h._DT[dtype]))


def conv_gru(h: torch.Tensor, x: torch.Tensor, w_zr: torch.Tensor, b_zr, w_q: torch.Tensor, b_q, KH: int, KW: int) -> torch.Tensor:
    """K17: one ConvGRU half (refinenet.py:7-36) on h, x (N,H,W,C) in one launch: (1 - z) * h + z * tanh(convq([r * h, x])) with
    z | r = sigmoid(conv([h, x])), KH x KW = 3 x 1 or 1 x 3.  w_zr: [convz | convr] stacked along Cout over cat(h, x), w_q: convq, both as K5 v5
    fragment streams (pack.pack_conv_frag); biases fp32 (2C) / (C) or None."""
    _h._resident("conv_gru", h, x, w_zr, b_zr, w_q, b_q)
    if h.dtype != torch.float16 or x.dtype != torch.float16 or tuple(h.shape) != tuple(x.shape):
        raise ValueError("conv_gru: h and x must be (N,H,W,C) fp16 tensors of one shape")
    hs, xs = _h._pixels(h, "conv_gru: h"), _h._pixels(x, "conv_gru: x")
    N, H, W, C = h.shape
    _h._vec(w_zr, 2 * C * KH * KW * 2 * C, "conv_gru: w_zr", dtype=h.dtype)
    _h._vec(w_q, C * KH * KW * 2 * C, "conv_gru: w_q", dtype=h.dtype)
    _h._vec(b_zr, 2 * C, "conv_gru: b_zr", optional=True)
    _h._vec(b_q, C, "conv_gru: b_q", optional=True)
    d = _h.ConvGruDesc()
    out = torch.empty((N, H, W, C), device=h.device, dtype=h.dtype)
    d.h, d.h_stride, d.x, d.x_stride, d.out, d.out_stride = h.data_ptr(), hs, x.data_ptr(), xs, out.data_ptr(), C
    d.N, d.H, d.W, d.C, d.KH, d.KW = N, H, W, C, KH, KW
    d.w_zr, d.w_q, d.b_zr, d.b_q, d.dtype = w_zr.data_ptr(), w_q.data_ptr(), _h._ptr(b_zr), _h._ptr(b_q), _h._DT[h.dtype]
    _h._check(_h.load().s2m2_conv_gru(ctypes.byref(d), _h._stream()), "s2m2_conv_gru")
    _h._meter("conv_gru", 2.0 * N * H * W * (3 * C) * (2 * C) * KH * KW)
    return out
