"""Engine files on the GPU (s2m2_amd/export.py, include/s2m2_hip.h: s2m2_plan_save / s2m2_engine_*): an exported forward, loaded by the library
and run without the Python model, returns exactly (torch.equal) what ``S2M2.forward`` returns for the same model and images -- in this process,
on other streams, with several engines loaded, and in a fresh process through the stand-alone ``s2m2_run_engine``.  Files damaged on purpose
are only ever LOADED (which must fail on the host); nothing is run from them."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from s2m2_amd.build import RUNNER
from s2m2_amd.export import NativeEngine, export_engine
from s2m2_amd.model import S2M2
from s2m2_amd.spec import MODEL_CONFIGS
from s2m2_amd.weights import seeded_state_dict, synthetic_pair

pytestmark = pytest.mark.gpu


def _model(kind, pos=True, up=False, ri=3, seed=0):
    C, ntr = MODEL_CONFIGS[kind]
    m = S2M2(C, 1, ntr, use_positivity=pos, output_upsample=up, refine_iter=ri)
    m.load_state_dict(seeded_state_dict(C, 1, ntr, seed), strict=True)
    return m.cuda().eval()


def _forward(m, l, r, dtype):
    if dtype == torch.float16:
        with torch.autocast("cuda", dtype=torch.float16):
            return m(l, r)
    return m(l, r)


def _pair(H, W, B=1, seed=0):
    l, r = synthetic_pair(H, W, B, 24, seed)
    return l.cuda().contiguous(), r.cuda().contiguous()


def _equal(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def s_engine(tmp_path_factory):
    """S 640x480 fp16, B = 1: the engine most tests share"""
    m = _model("S")
    path = str(tmp_path_factory.mktemp("engine") / "s_480x640_fp16.s2m2")
    info = export_engine(m, path, 480, 640)
    return m, path, info


CASES = [
    ("S", 480, 640, 1, torch.float16, {}),
    ("S", 480, 640, 1, torch.float32, {}),
    ("S", 1024, 1216, 1, torch.float16, {}),                         # the bench configuration
    ("M", 480, 640, 1, torch.float16, {}),                           # 192-channel forms
    ("L", 1024, 1216, 1, torch.float16, {}),                         # the 512-channel direct K9 / K10 forms
    ("XL", 480, 640, 1, torch.float16, {}),
    ("S", 480, 640, 1, torch.float16, {"pos": False, "up": True, "ri": 1}),
    ("S", 480, 640, 2, torch.float16, {}),
]


@pytest.mark.parametrize("kind,H,W,B,dtype,opts", CASES, ids=[f"{c[0]}-{c[2]}x{c[1]}-b{c[3]}-{str(c[4])[6:]}-{i}" for i, c in enumerate(CASES)])
def test_engine_is_bit_identical_to_the_forward(tmp_path, monkeypatch, kind, H, W, B, dtype, opts):
    # the engine is the batched forward: pair side streams off (they are out of scope for engines; with them the batch runs as B single-pair forwards)
    monkeypatch.setenv("S2M2_PAIR_STREAMS", "0")
    m = _model(kind, **opts)
    path = str(tmp_path / "e.s2m2")
    info = export_engine(m, path, H, W, batch=B, dtype=dtype)
    assert info["launches"] > 100 and info["bytes"] == os.path.getsize(path)
    eng = NativeEngine(path)
    assert eng.meta["out_shape"] == (B, 1, 2 * H if opts.get("up") else H, 2 * W if opts.get("up") else W)
    assert eng.meta["dtype"] == dtype and eng.meta["feature_channels"] == MODEL_CONFIGS[kind][0]
    l, r = _pair(H, W, B)
    ref = _forward(m, l, r, dtype)
    first = eng.run(l, r)                                            # eager
    second = eng.run(l, r)                                           # captured as a hipGraph and replayed
    torch.cuda.synchronize()
    assert _equal(first, ref) and _equal(second, ref)


def test_runs_rebind_their_inputs_and_carry_no_state(s_engine):
    m, path, _ = s_engine
    eng = NativeEngine(path)
    pairs = [_pair(480, 640, 1, s) for s in (1, 2, 3)]
    refs = [_forward(m, l, r, torch.float16) for l, r in pairs]
    assert not torch.equal(refs[0][0], refs[1][0])
    for k in (0, 1, 2, 0):
        out = eng.run(*pairs[k])
        torch.cuda.synchronize()
        assert _equal(out, refs[k]), k


def test_non_default_stream_and_two_engines(s_engine):
    m, path, _ = s_engine
    a, b = NativeEngine(path), NativeEngine(path)
    l, r = _pair(480, 640, 1, 7)
    ref = _forward(m, l, r, torch.float16)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        outs = [e.run(l, r) for e in (a, b, a, b, a, b)]
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert all(_equal(o, ref) for o in outs)


def test_fresh_process_runner_is_bit_identical(s_engine, tmp_path):
    m, path, _ = s_engine
    l, r = _pair(480, 640, 1, 11)
    ref = _forward(m, l, r, torch.float16)
    lp, rp = tmp_path / "left.f32", tmp_path / "right.f32"
    lp.write_bytes(l.cpu().numpy().astype("<f4").tobytes())
    rp.write_bytes(r.cpu().numpy().astype("<f4").tobytes())
    p = subprocess.run([RUNNER, path, str(lp), str(rp), "--out", str(tmp_path), "--repeat", "3"], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr
    assert "ms_per_pair" in p.stdout
    for name, t in zip(("disp", "occ", "conf"), ref):
        got = torch.from_numpy(np.fromfile(tmp_path / f"{name}.f32", dtype="<f4").reshape(tuple(t.shape)))
        assert torch.equal(got, t.cpu()), name


# file layout (s2m2_amd/csrc/engine_file.hip): header, then regions (24 bytes), calls (96 bytes: name[48] first), patches (24 bytes)
_HDR = struct.Struct("<8sIIIIIIQQ")
_HDR_BYTES = 112


def _tables(blob):
    _, _, _, nreg, ncall, npatch, _, _, _ = _HDR.unpack_from(blob, 0)
    calls = _HDR_BYTES + 24 * nreg
    patches = calls + 96 * ncall
    return nreg, ncall, npatch, calls, patches


def _load_fails(path, what):
    with pytest.raises(RuntimeError, match=what):
        NativeEngine(path)


def test_damaged_files_fail_to_load(s_engine, tmp_path):
    _, path, _ = s_engine
    blob = open(path, "rb").read()
    nreg, ncall, npatch, calls, patches = _tables(blob)
    assert len(blob) > patches + 24 * npatch and npatch > 0
    # an entry name flipped
    bad = bytearray(blob)
    k = calls + 96 * (ncall // 2)
    assert bad[k:k + 5] == b"s2m2_"
    bad[k + 5] ^= 0x20
    (tmp_path / "name.s2m2").write_bytes(bytes(bad))
    _load_fails(str(tmp_path / "name.s2m2"), "unknown entry point")
    # truncated
    (tmp_path / "short.s2m2").write_bytes(blob[:len(blob) - 4096])
    _load_fails(str(tmp_path / "short.s2m2"), "bytes, the header describes")
    # a patch offset moved past the end of its region
    bad = bytearray(blob)
    q = patches + 24 * (npatch // 2)
    region = struct.unpack_from("<I", bad, q + 8)[0]
    rbytes = struct.unpack_from("<Q", bad, _HDR_BYTES + 24 * region + 8)[0]
    struct.pack_into("<Q", bad, q + 16, rbytes)
    (tmp_path / "patch.s2m2").write_bytes(bytes(bad))
    _load_fails(str(tmp_path / "patch.s2m2"), "outside region")
