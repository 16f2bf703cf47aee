"""CPU-side checks of K17's boundary (s2m2_conv_gru): descriptor layout against the header, argument validation before any device call, the
wrapper's operand checks, the loader table of engine files.  The kernel itself: tests/test_hip_conv_gru.py."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from s2m2_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16 = torch.float16


@pytest.fixture(scope="module")
def lib():
    from s2m2_amd.build import build
    build(verbose=False)
    return hip.load()


def test_descriptor_has_the_layout_of_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = [f[0] for f in hip.ConvGruDesc._fields_]
    body = "".join(f'  printf("%zu\\n", offsetof(s2m2_convgru_desc, {f}));\n' for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s2m2_hip.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(s2m2_convgru_desc));\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(hip.ConvGruDesc)
    assert out[1:] == [getattr(hip.ConvGruDesc, f).offset for f in fields]


HP, XP, OUT = 1 << 20, 2 << 20, 3 << 20                            # far enough apart for the byte ranges of 8 x 20 x 128 tensors
SPAN = 8 * 20 * 128 * 2


def _desc(**kw):
    d = hip.ConvGruDesc()
    d.h, d.x, d.out, d.w_zr, d.w_q = HP, XP, OUT, 4096, 4096
    d.h_stride = d.x_stride = d.out_stride = 128
    d.N, d.H, d.W, d.C, d.KH, d.KW, d.dtype = 1, 8, 20, 128, 3, 1, hip.F16
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_validation_runs_before_any_device_call(lib):
    assert lib.s2m2_conv_gru_supported(128, 256, 304, hip.F16) == 1 and lib.s2m2_conv_gru_supported(128, 1, 1, hip.F16) == 1
    assert lib.s2m2_conv_gru_supported(256, 256, 304, hip.F16) == 0 and lib.s2m2_conv_gru_supported(128, 256, 304, hip.F32) == 0
    assert lib.s2m2_conv_gru_supported(128, 0, 304, hip.F16) == 0
    assert lib.s2m2_conv_gru(None, None) != 0 and b"null descriptor" in lib.s2m2_last_error()
    for kw, msg in (({"C": 64}, b"C=64"), ({"dtype": hip.F32}, b"fp16"), ({"KH": 3, "KW": 3}, b"3 x 1 or 1 x 3"), ({"KH": 1, "KW": 1}, b"3 x 1 or 1 x 3"),
                    ({"x": None}, b"x is null"), ({"out": HP}, b"out aliases h"), ({"out": XP}, b"out aliases x"), ({"H": 0}, b"bad shape"),
                    ({"N": 1 << 12, "H": 1 << 6, "W": 1 << 6}, b"bad shape"), ({"h_stride": 120}, b"h_stride=120"), ({"x_stride": 132}, b"x_stride=132"),
                    ({"out_stride": 64}, b"out_stride=64"), ({"h": HP + 4}, b"h must be 16-byte aligned"), ({"w_q": None}, b"w_q is null"),
                    ({"w_zr": None}, b"w_zr is null"),
                    ({"out": HP + SPAN - 16}, b"out aliases h"),          # out starts on the last 16 bytes of h
                    ({"out": XP - SPAN + 16}, b"out aliases x")):         # out ends 16 bytes into x
        assert lib.s2m2_conv_gru(ctypes.byref(_desc(**kw)), None) != 0, kw
        assert msg in lib.s2m2_last_error(), (kw, lib.s2m2_last_error())


class _NoLibrary:
    def __getattr__(self, name):
        pytest.fail(f"the binding reached the library ({name})")


def test_the_wrapper_checks_its_operands_before_the_library_is_touched(monkeypatch):
    monkeypatch.setattr(hip, "_lib", _NoLibrary())
    h = torch.zeros(1, 4, 40, 128, dtype=F16)
    w_zr, w_q = torch.zeros(256 * 256 * 3, dtype=F16), torch.zeros(128 * 256 * 3, dtype=F16)
    with pytest.raises(ValueError, match="device tensors"):
        hip.conv_gru(h, h, w_zr, None, w_q, None, 1, 3)
    assert hip.conv_gru.__doc__ and hip.conv_gru_supported.__doc__


def test_the_engine_file_loader_knows_the_entry_point(lib, tmp_path):
    """s2m2_conv_gru is in the table engine files are loaded through, with the blob size of its descriptor: a file that names it with a
    one-word blob is refused for the size, not as an unknown entry point"""
    import test_engine_file_cpu as EF
    msg = EF._fails(lib, tmp_path, EF._file("s2m2_conv_gru", 1), r"\(s2m2_conv_gru\) has a blob of 1 words, the entry point takes \d+")
    words = int(msg.split("the entry point takes")[1].split()[0])
    assert words * 8 == 8 + ctypes.sizeof(hip.ConvGruDesc), (words, ctypes.sizeof(hip.ConvGruDesc))    # impl pointer + descriptor
