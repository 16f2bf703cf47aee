"""CPU-side checks of engine files (include/s2m2_hip.h: s2m2_engine_load, s2m2_plan_save; s2m2_amd/csrc/engine_file.hip): a malformed or foreign
file is refused by s2m2_engine_load with a message, on the host, before any device call -- this container has no GPU, so a load that got as far
as the device would fail with a different message.  Also: the ctypes mirrors of the new structs, the table of recordable entry points the loader
maps names through, and the stand-alone runner's error path."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import pytest

from s2m2_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "s2m2_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from s2m2_amd.build import build
    build(verbose=False)
    return hip.load()


def _header(magic=b"S2M2ENG\0", fmt=1, abi=None, nreg=3, ncall=1, npatch=0, arena=1, data=0, info=None):
    if info is None:
        info = hip.EngineInfo()
        info.B, info.H, info.W, info.dtype, info.image_dtype = 1, 32, 32, hip.F16, 0
        info.feature_channels, info.dim_expansion, info.num_transformer, info.refine_iter = 128, 1, 1, 1
        info.out_h, info.out_w, info.out_region, info.out_offset = 32, 32, 2, 0
    head = struct.pack("<8sIIIIIIQQ", magic, fmt, hip.ABI_VERSION if abi is None else abi, nreg, ncall, npatch, ctypes.sizeof(info), arena, data)
    return head + bytes(info)


def _file(name, words=1):
    """a well-formed engine file around ONE call to entry point `name` with a blob of `words` words (nothing stored: every region is scratch
    or an image)"""
    img = 3 * 32 * 32 * 4
    regions = struct.pack("<IIQQ", hip.REGION_EXTERNAL, 0, img, 0) * 2 + struct.pack("<IIQQ", hip.REGION_SCRATCH, 0, 3 * 32 * 32 * 4, 0)
    call = name.encode().ljust(48, b"\0") + struct.pack("<IIQ", words, 0, 0) + bytes(32)
    return _header(arena=words) + regions + call + bytes(8 * words)


def _fails(lib, tmp_path, blob, what):
    p = tmp_path / "e.s2m2"
    p.write_bytes(blob)
    h = ctypes.c_void_p()
    assert lib.s2m2_engine_load(str(p).encode(), ctypes.byref(h)) != 0 and not h
    msg = lib.s2m2_last_error().decode()
    assert re.search(what, msg), msg
    return msg


def test_load_refuses_missing_foreign_and_truncated_files(lib, tmp_path):
    h = ctypes.c_void_p()
    assert lib.s2m2_engine_load(str(tmp_path / "absent.s2m2").encode(), ctypes.byref(h)) != 0
    assert b"cannot open" in lib.s2m2_last_error()
    good = _file("s2m2_tanh", 1)
    _fails(lib, tmp_path, b"GGUF" + good[4:], "bad magic")
    _fails(lib, tmp_path, _header(abi=600) + good[len(_header()):], "ABI version 600")
    _fails(lib, tmp_path, _header(fmt=9) + good[len(_header()):], "format version 9")
    _fails(lib, tmp_path, good[:50], "truncated header")
    _fails(lib, tmp_path, good[:-8], "the header describes")
    _fails(lib, tmp_path, good + b"\0" * 8, "the header describes")


def test_load_refuses_unknown_entry_points_and_wrong_blob_sizes(lib, tmp_path):
    _fails(lib, tmp_path, _file("s2m2_not_an_entry_point"), "unknown entry point 's2m2_not_an_entry_point'")
    for name in _recorded_names():
        _fails(lib, tmp_path, _file(name, 1), rf"\({name}\) has a blob of 1 words, the entry point takes \d+")


def _recorded_names():
    names = set()
    for f in os.listdir(CSRC):
        if f.endswith(".hip"):
            names |= set(re.findall(r'plan_dispatch(?:_desc)?(?:<\w+>)?\("(s2m2_\w+)"', open(os.path.join(CSRC, f)).read()))
    return sorted(names)


def test_every_recorded_entry_point_is_in_the_loader_table():
    """plan_dispatch names (what a recording stores) against the S2M2_PLAN_ENTRY registrations (what the loader maps names back through)"""
    registered = []
    for f in os.listdir(CSRC):
        if f.endswith(".hip"):
            src = open(os.path.join(CSRC, f)).read()
            for name, impl in re.findall(r'^S2M2_PLAN(?:_DESC)?_ENTRY\("(s2m2_\w+)", (\w+)\)', src, flags=re.M):
                registered.append(name)
                assert re.search(rf'plan_dispatch(?:_desc)?(?:<\w+>)?\("{name}", &{impl}\b', src), (f, name, impl)
    assert sorted(registered) == _recorded_names()
    assert len(registered) == 22                                      # K14, K17 and K19 register through a constant: their own *_cpu.py tests


def test_engine_structs_have_the_layout_of_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    pairs = [("s2m2_engine_region", hip.EngineRegion), ("s2m2_engine_info", hip.EngineInfo)]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "s2m2_hip.h"', "int main(void) {"]
    for cname, py in pairs:
        for f in py._fields_:
            lines.append(f'  printf("{cname} {f[0]} %zu %zu\\n", sizeof({cname}), offsetof({cname}, {f[0]}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [(c, py, f[0]) for c, py in pairs for f in py._fields_]
    for (cname, py, field), line in zip(rows, out):
        name, fname, size, off = line.split()
        assert (name, fname) == (cname, field)
        assert int(size) == ctypes.sizeof(py) and int(off) == getattr(py, field).offset, (cname, field)


def test_runner_reports_the_library_message_for_a_missing_file(lib, tmp_path):
    from s2m2_amd.build import RUNNER
    assert os.path.exists(RUNNER)
    p = subprocess.run([RUNNER, str(tmp_path / "absent.s2m2"), "l.f32", "r.f32"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0
    assert "engine_load: cannot open" in p.stderr and "absent.s2m2" in p.stderr


def test_native_engine_raises_on_a_missing_file(lib, tmp_path):
    from s2m2_amd.export import NativeEngine
    with pytest.raises(RuntimeError, match="cannot open"):
        NativeEngine(str(tmp_path / "absent.s2m2"))
