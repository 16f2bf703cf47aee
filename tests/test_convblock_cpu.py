"""CPU-side checks of K14's boundary (s2m2_conv_block): descriptor layout against the header, argument validation before any device call (one
refused descriptor per rule of the shared operand validators, csrc/launch.h), the loader table of engine files.  The kernel itself:
tests/test_hip_convblock.py."""
import ctypes
import os
import shutil
import subprocess

import pytest

from s2m2_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from s2m2_amd.build import build
    build(verbose=False)
    return hip.load()


def _compiler():
    for cc in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cc)
        if path:
            return path
    raise RuntimeError("no host C++ compiler found (c++, g++, clang++)")


def test_descriptor_has_the_layout_of_the_header(tmp_path):
    fields = [f[0] for f in hip.ConvBlockDesc._fields_]
    body = "".join(f'  printf("%zu\\n", offsetof(s2m2_convblock_desc, {f}));\n' for f in fields)
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s2m2_hip.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(s2m2_convblock_desc));\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([_compiler(), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(hip.ConvBlockDesc)
    assert out[1:] == [getattr(hip.ConvBlockDesc, f).offset for f in fields]


X, OUT = 1 << 20, 2 << 20
SPAN = 4 * 40 * 128 * 2                                           # bytes of one 4 x 40 x 128 tensor


def _desc(**kw):
    d = hip.ConvBlockDesc()
    d.x, d.out, d.w_conv0, d.w_conv2, d.w_1x0, d.w_1x2 = X, OUT, 4096, 4096, 4096, 4096
    d.x_stride = d.out_stride = 128
    d.N, d.H, d.W, d.C, d.dtype = 1, 4, 40, 128, hip.F16
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_supported_predicate(lib):
    assert lib.s2m2_conv_block_supported(128, 128, 152, hip.F16) == 1 and lib.s2m2_conv_block_supported(256, 1, 1, hip.F16) == 1
    assert lib.s2m2_conv_block_supported(128, 160, 192, hip.F16) == 1                                 # H * W <= 160 * 192: the bound itself ...
    assert lib.s2m2_conv_block_supported(128, 160, 193, hip.F16) == 0 and lib.s2m2_conv_block_supported(128, 161, 192, hip.F16) == 0   # ... and past it
    assert lib.s2m2_conv_block_supported(64, 64, 76, hip.F16) == 0 and lib.s2m2_conv_block_supported(192, 64, 76, hip.F16) == 0
    assert lib.s2m2_conv_block_supported(128, 64, 76, hip.F32) == 0 and lib.s2m2_conv_block_supported(128, 0, 76, hip.F16) == 0


def test_argument_validation_runs_before_any_device_call(lib):
    assert lib.s2m2_conv_block(None, None) != 0 and b"null descriptor" in lib.s2m2_last_error()
    for kw, msg in (({"x": None}, b"x is null"), ({"out": None}, b"out is null"), ({"w_conv0": None}, b"w_conv0 is null"),
                    ({"w_conv2": None}, b"w_conv2 is null"), ({"w_1x0": None}, b"w_1x0 is null"), ({"w_1x2": None}, b"w_1x2 is null"),
                    ({"dtype": hip.F32}, b"fp16"), ({"C": 64}, b"C=64"), ({"C": 192}, b"C=192"),
                    ({"H": 0}, b"bad shape"), ({"N": 1 << 12, "H": 1 << 6, "W": 1 << 6}, b"bad shape"),
                    ({"x": X + 4}, b"x must be 16-byte aligned"), ({"out": OUT + 4}, b"out must be 8-byte aligned"),
                    ({"w_1x0": 4100}, b"w_1x0 must be 16-byte aligned"),
                    ({"x_stride": 120}, b"x_stride=120"), ({"x_stride": 132}, b"x_stride=132"), ({"out_stride": 130}, b"out_stride=130"),
                    ({"out": X}, b"out aliases x"),
                    ({"out": X + SPAN - 16}, b"out aliases x"),           # out starts on the last 16 bytes of x
                    ({"out": X - SPAN + 16}, b"out aliases x")):          # out ends 16 bytes into x
        assert lib.s2m2_conv_block(ctypes.byref(_desc(**kw)), None) != 0, kw
        err = lib.s2m2_last_error()
        assert err.startswith(b"conv_block: ") and msg in err, (kw, err)


def test_dispatch_and_registration_share_one_name():
    text = open(os.path.join(ROOT, "s2m2_amd", "csrc", "convblock.hip")).read()
    assert text.count('"s2m2_conv_block"') == 1                       # the constant; dispatch and registration both go through it
    assert "plan_dispatch_desc<s2m2_convblock_desc>(kConvBlockEntry" in text and "S2M2_PLAN_DESC_ENTRY(kConvBlockEntry" in text


def test_the_engine_file_loader_knows_the_entry_point(lib, tmp_path):
    """s2m2_conv_block is in the table engine files are loaded through, with the blob size of its descriptor: a file that names it with a
    one-word blob is refused for the size, not as an unknown entry point"""
    import test_engine_file_cpu as EF
    msg = EF._fails(lib, tmp_path, EF._file("s2m2_conv_block", 1), r"\(s2m2_conv_block\) has a blob of 1 words, the entry point takes \d+")
    words = int(msg.split("the entry point takes")[1].split()[0])
    assert words * 8 == 8 + ctypes.sizeof(hip.ConvBlockDesc), (words, ctypes.sizeof(hip.ConvBlockDesc))    # impl pointer + descriptor
