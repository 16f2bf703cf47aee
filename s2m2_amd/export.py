"""Engine files: one forward of an ``S2M2`` model with fixed settings -- weights, batch, height, width, compute dtype, image dtype -- written to
disk as a self-contained file that ``libs2m2_hip.so`` loads and runs without Python (include/s2m2_hip.h: s2m2_plan_save, s2m2_engine_*;
``s2m2_amd/app/run_engine.cpp`` is a stand-alone C++ caller).  This project's counterpart of the reference's TensorRT engine export, built from
the project's own kernels.

* :func:`export_engine` records one forward with the library's launch plans (s2m2_plan_begin / end) and hands the library the memory that
  forward touched, as regions: the engine's persistent tensors (parameters, packed weights and fragment streams, PE tables, LayerNorm row sums,
  the zero-initialised scratch of ``Engine.zeros``) are *content*; the transient tensors are *scratch*, taken by allocator segment of the
  private ``MemPool`` the forward was recorded in -- so the caching allocator's reuse of freed blocks inside the forward is kept exactly as
  recorded; the two images are the *externals*.  The file format is the library's: nothing here parses or writes it.
* :class:`NativeEngine` is a thin ctypes wrapper around a loaded engine file (tests, and Python users of the same file).
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, Tuple

import torch
from torch.utils._python_dispatch import TorchDispatchMode

from . import hip
from .engine import Engine, Layer, check_limits, max_batch

_IMG_DT = {torch.float32: 0, torch.float16: 1, torch.uint8: 2}
_IMG_FROM = {v: k for k, v in _IMG_DT.items()}
_DT_FROM = {hip.F32: torch.float32, hip.F16: torch.float16}

# tensor ops that launch nothing: allocations and views (a recorded forward must consist of library calls only -- a torch kernel between two
# of them would be missing from the plan)
_NO_KERNEL = {"empty", "empty_strided", "empty_like", "new_empty", "new_empty_strided", "detach", "alias", "lift_fresh", "split",
              "split_with_sizes", "unbind", "chunk", "_unsafe_view", "_reshape_alias"}


class _TorchKernels(TorchDispatchMode):
    """lists every tensor op inside the block that is neither an allocation nor a view"""

    def __init__(self):
        super().__init__()
        self.ops: List[str] = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if not (func.is_view or func.overloadpacket.__name__ in _NO_KERNEL):
            self.ops.append(str(func))
        return func(*args, **(kwargs or {}))


def _storages(obj, out: Dict[int, int], seen: set) -> None:
    """device storages (base pointer -> bytes) reachable from obj through dicts, lists, tuples and the engine's packed layers (a Layer's
    weight, bias and the derived packings it has built so far)"""
    if isinstance(obj, torch.Tensor):
        if obj.is_cuda:
            st = obj.untyped_storage()
            if st.nbytes():
                out[st.data_ptr()] = st.nbytes()
        return
    if id(obj) in seen:
        return
    seen.add(id(obj))
    if isinstance(obj, dict):
        for v in obj.values():
            _storages(v, out, seen)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _storages(v, out, seen)
    elif isinstance(obj, Layer):
        _storages(vars(obj), out, seen)


def _engine_storages(eng: Engine) -> Dict[int, int]:
    out: Dict[int, int] = {}
    _storages(list(eng.__dict__.values()), out, set())
    return out


def _images(B: int, H: int, W: int, dtype: torch.dtype, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """two distinct deterministic images in [0, 255] (the recorded run's content does not matter; their extents do)"""
    g = torch.Generator(device="cpu").manual_seed(0)
    left = (torch.rand((B, 3, H, W), generator=g) * 255).to(dtype).to(dev)
    right = (torch.rand((B, 3, H, W), generator=g) * 255).to(dtype).to(dev)
    return left.contiguous(), right.contiguous()


def export_engine(model, path: str, height: int, width: int, batch: int = 1, dtype: torch.dtype = torch.float16,
                  image_dtype: torch.dtype = torch.float32) -> dict:
    """Write the forward of ``model`` for (batch, 3, height, width) images of ``image_dtype`` at compute ``dtype`` to ``path``.  The model must
    be on a MI355X; the engine returns what ``model(left, right)`` returns for such images (under ``torch.autocast(float16)`` for fp16).
    Returns a summary: launches, regions by kind, file bytes."""
    if dtype not in (torch.float16, torch.float32):
        raise ValueError(f"export_engine: compute dtype {dtype} (float16 or float32)")
    if image_dtype not in _IMG_DT:
        raise ValueError(f"export_engine: image dtype {image_dtype} (float32, float16 or uint8)")
    p0 = next(model.parameters())
    if not p0.is_cuda:
        raise RuntimeError("export_engine: move the model to a CUDA(HIP) device first (engines are recorded on the MI355X they run on)")
    H, W, B = int(height), int(width), int(batch)
    if H % 32 or W % 32 or H <= 0 or W <= 0 or B <= 0:
        raise ValueError("export_engine: height and width must be positive multiples of 32 and batch positive")
    if hip.METER is not None or hip.ATTN_EVENTS is not None or hip.ROW_EVENTS is not None:
        raise RuntimeError("export_engine: the work meter / attention timing events are on (they attach host state to launches)")
    dev = p0.device
    with model._lock, torch.cuda.device(dev), torch.no_grad(), torch.autocast("cuda", enabled=False):
        check_limits(H, W, model.feature_channels, B, dtype, use_pe="feat_pyramid.enc3s.0.self_attn.attn.pe_proj.weight" in model._table)
        nb = max_batch(H, W)
        if B > nb:
            raise ValueError(f"export_engine: batch {B} exceeds the {nb} pairs one forward takes at {H}x{W}")
        # a private Engine: the model's own engines, graphs and plans are left as they are
        eng = Engine(model, dtype)
        eng.native_refine = False            # s2m2_plan_run refuses to run while a plan records: refinement enqueued from Python
        if eng.k1_events is not None:
            raise RuntimeError("export_engine: K1 timing events are host handles and cannot go into a file")
        left, right = _images(B, H, W, image_dtype, dev)
        for _ in range(2):                   # warm-up: weights packed, persistent scratch allocated, lazy library state set up
            eng.run(left, right)
        torch.cuda.synchronize(dev)
        before = _engine_storages(eng)
        before_tokens = eng._tokens_normed
        pool = torch.cuda.MemPool()
        plan = hip.Plan()
        guard = _TorchKernels()
        with torch.cuda.use_mem_pool(pool, device=dev):
            with guard, plan.record([]):
                out = eng.run(left, right)
        torch.cuda.synchronize(dev)
        if guard.ops:
            raise RuntimeError("export_engine: the forward ran tensor ops outside the kernel library, which a plan cannot record: "
                               + ", ".join(sorted(set(guard.ops))))

        segs = sorted((s["address"], s["total_size"]) for s in pool.snapshot() if s.get("device", dev.index) == dev.index)
        inside = lambda p: any(a <= p < a + n for a, n in segs)                           # noqa: E731
        after = _engine_storages(eng)
        tokens = eng._tokens_normed
        new = {p for p in after if p not in before and not (tokens is not None and p == tokens.untyped_storage().data_ptr())}
        del before_tokens
        if new:
            raise RuntimeError(f"export_engine: the recorded forward created {len(new)} persistent engine tensors (warm-up incomplete)")
        img = {left.data_ptr(), right.data_ptr()}
        regions = [(left.data_ptr(), left.numel() * left.element_size(), hip.REGION_EXTERNAL),
                   (right.data_ptr(), right.numel() * right.element_size(), hip.REGION_EXTERNAL)]
        regions += [(p, n, hip.REGION_CONTENT) for p, n in sorted(after.items()) if not inside(p) and p not in img]
        first_seg = len(regions)
        regions += [(a, n, hip.REGION_SCRATCH) for a, n in segs]

        base = out[0]._base if out[0]._base is not None else out[0]
        if any(o.data_ptr() != base.data_ptr() + k * o.numel() * 4 for k, o in enumerate(out)) or out[0].dtype != torch.float32:
            raise RuntimeError("export_engine: the forward's three maps are not one (3, B, 1, H, W) fp32 allocation")
        optr = base.data_ptr()
        k = next((i for i, (a, n) in enumerate(segs) if a <= optr < a + n), None)
        if k is None:
            raise RuntimeError("export_engine: the forward's result is not in the recording pool")
        oh, ow = out[0].shape[-2:]

        info = hip.EngineInfo()
        info.B, info.H, info.W, info.dtype, info.image_dtype = B, H, W, hip._DT[dtype], _IMG_DT[image_dtype]
        info.feature_channels, info.dim_expansion, info.num_transformer = model.feature_channels, model.dim_expansion, model.num_transformer
        info.use_positivity, info.output_upsample, info.refine_iter = int(model.use_positivity), int(model.output_upsample), model.refine_iter
        info.out_h, info.out_w, info.out_region, info.out_offset = oh, ow, first_seg + k, optr - segs[k][0]
        arr = (hip.EngineRegion * len(regions))()
        for i, (a, n, kind) in enumerate(regions):
            arr[i].base, arr[i].bytes, arr[i].kind = a, n, kind
        hip._check(hip.load().s2m2_plan_save(plan.h, arr, len(regions), ctypes.byref(info), os.fsencode(path)), "s2m2_plan_save")
        launches = plan.launches
        del out, plan, pool
    return {"launches": launches, "content_regions": first_seg - 2, "scratch_regions": len(segs), "bytes": os.path.getsize(path)}


class NativeEngine:
    """An engine file loaded on the current device (s2m2_engine_load).  ``run(left, right) -> (disp, occ, conf)``: (B,3,H,W) images of the
    engine's image dtype on that device -> three (B,1,out_h,out_w) fp32 maps, enqueued on the current stream.  One run at a time per engine."""

    def __init__(self, path: str):
        lib = hip.load()
        self.h = ctypes.c_void_p()
        hip._check(lib.s2m2_engine_load(os.fsencode(path), ctypes.byref(self.h)), "s2m2_engine_load")
        self.device = torch.device("cuda", torch.cuda.current_device())
        info = hip.EngineInfo()
        hip._check(lib.s2m2_engine_meta(self.h, ctypes.byref(info)), "s2m2_engine_meta")
        self.meta = {"B": info.B, "H": info.H, "W": info.W, "dtype": _DT_FROM[info.dtype], "image_dtype": _IMG_FROM[info.image_dtype],
                     "feature_channels": info.feature_channels, "dim_expansion": info.dim_expansion, "num_transformer": info.num_transformer,
                     "use_positivity": bool(info.use_positivity), "output_upsample": bool(info.output_upsample), "refine_iter": info.refine_iter,
                     "out_shape": (info.B, 1, info.out_h, info.out_w)}

    def run(self, left: torch.Tensor, right: torch.Tensor):
        m = self.meta
        want = (m["B"], 3, m["H"], m["W"])
        for t in (left, right):
            if tuple(t.shape) != want or t.dtype != m["image_dtype"] or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"NativeEngine.run: images must be contiguous {want} {m['image_dtype']} tensors on {self.device}, "
                                 f"got {tuple(t.shape)} {t.dtype} on {t.device}")
        outs = [torch.empty(m["out_shape"], device=self.device, dtype=torch.float32) for _ in range(3)]
        with torch.cuda.device(self.device):
            hip._check(hip.load().s2m2_engine_run(self.h, left.data_ptr(), right.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                                  outs[2].data_ptr(), torch.cuda.current_stream(self.device).cuda_stream), "s2m2_engine_run")
        return tuple(outs)

    def close(self) -> None:
        if self.h:
            hip.load().s2m2_engine_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass
