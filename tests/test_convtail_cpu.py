"""CPU-side checks of K19's boundary (s2m2_conv_block_tail): descriptor layout against the header, argument validation before any device call, the
loader table of engine files, and the patch rule (csrc/convtail_select.h) as a pure function held against K5's choice for the launch it replaces.
The kernel itself: tests/test_hip_convtail.py."""
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


def _compiler():
    for cc in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cc)
        if path:
            return path
    raise RuntimeError("no host C++ compiler found (c++, g++, clang++)")


def test_descriptor_has_the_layout_of_the_header(tmp_path):
    fields = [f[0] for f in hip.ConvTailDesc._fields_]
    body = "".join(f'  printf("%zu\\n", offsetof(s2m2_convtail_desc, {f}));\n' for f in fields)
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s2m2_hip.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(s2m2_convtail_desc));\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([_compiler(), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(hip.ConvTailDesc)
    assert out[1:] == [getattr(hip.ConvTailDesc, f).offset for f in fields]


def _desc(**kw):
    d = hip.ConvTailDesc()
    d.t, d.z, d.out, d.w_conv2, d.w_1x0, d.w_1x2 = 1 << 20, 2 << 20, 3 << 20, 4096, 4096, 4096
    d.t_stride = d.z_stride = d.out_stride = 128
    d.N, d.H, d.W, d.C, d.dtype = 1, 4, 40, 128, hip.F16
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_validation_runs_before_any_device_call(lib):
    assert lib.s2m2_conv_block_tail_supported(128, 256, 304, hip.F16) == 1 and lib.s2m2_conv_block_tail_supported(256, 1, 1, hip.F16) == 1
    assert lib.s2m2_conv_block_tail_supported(64, 64, 76, hip.F16) == 0 and lib.s2m2_conv_block_tail_supported(192, 64, 76, hip.F16) == 0
    assert lib.s2m2_conv_block_tail_supported(128, 64, 76, hip.F32) == 0 and lib.s2m2_conv_block_tail_supported(128, 0, 76, hip.F16) == 0
    assert lib.s2m2_conv_block_tail(None, None) != 0 and b"null descriptor" in lib.s2m2_last_error()
    span = 160 * 128 * 2                                          # bytes of one 4 x 40 x 128 tensor
    for kw, msg in (({"t": None}, b"t is null"), ({"z": None}, b"z is null"), ({"out": None}, b"out is null"), ({"w_conv2": None}, b"w_conv2 is null"),
                    ({"w_1x0": None}, b"w_1x0 is null"), ({"w_1x2": None}, b"w_1x2 is null"), ({"dtype": hip.F32}, b"fp16 only"), ({"C": 64}, b"C=64"),
                    ({"C": 192}, b"C=192"), ({"H": 0}, b"bad shape"), ({"N": 1 << 12, "H": 1 << 6, "W": 1 << 6}, b"bad shape"),
                    ({"t_stride": 120}, b"t_stride=120"), ({"z_stride": 132}, b"z_stride=132"), ({"out_stride": 129}, b"out_stride=129"),
                    ({"t": (1 << 20) + 4}, b"t must be 16-byte aligned"), ({"N": 1 << 10, "H": 1 << 6, "W": 1 << 6, "z_stride": 1 << 10}, b"z spans 2^31"),
                    ({"out": 1 << 20}, b"out aliases t"), ({"out": 2 << 20}, b"out aliases z"),
                    ({"out": (1 << 20) + span - 16}, b"out aliases t"), ({"out": (2 << 20) - span + 16}, b"out aliases z"),
                    ({"patch_rows": 4, "patch_cols": 36}, b"patch 4 x 36"), ({"patch_rows": 2}, b"patch 2 x 0")):
        assert lib.s2m2_conv_block_tail(ctypes.byref(_desc(**kw)), None) != 0, kw
        assert msg in lib.s2m2_last_error(), (kw, lib.s2m2_last_error())


class _NoLibrary:
    def __getattr__(self, name):
        pytest.fail(f"the binding reached the library ({name})")


def test_the_wrapper_checks_its_operands_before_the_library_is_touched(monkeypatch):
    monkeypatch.setattr(hip, "_lib", _NoLibrary())
    t = torch.zeros(1, 4, 40, 128, dtype=F16)
    w2, w1 = torch.zeros(9 * 128 * 128, dtype=F16), torch.zeros(128 * 128, dtype=F16)
    with pytest.raises(ValueError, match="device tensors"):
        hip.conv_block_tail(t, t, w2, None, w1, None, w1, None)
    assert hip.conv_block_tail.__doc__ and hip.conv_block_tail_supported.__doc__
    assert hip.conv_block_tail.__module__ == "s2m2_amd.hip_tail"


def test_the_engine_file_loader_knows_the_entry_point(lib, tmp_path):
    """s2m2_conv_block_tail is in the table engine files are loaded through, with the blob size of its descriptor: a file that names it with a
    one-word blob is refused for the size, not as an unknown entry point"""
    import test_engine_file_cpu as EF
    msg = EF._fails(lib, tmp_path, EF._file("s2m2_conv_block_tail", 1), r"\(s2m2_conv_block_tail\) has a blob of 1 words, the entry point takes \d+")
    words = int(msg.split("the entry point takes")[1].split()[0])
    assert words * 8 == 8 + ctypes.sizeof(hip.ConvTailDesc), (words, ctypes.sizeof(hip.ConvTailDesc))    # impl pointer + descriptor


def test_dispatch_and_registration_share_one_name():
    text = open(os.path.join(ROOT, "s2m2_amd", "csrc", "convtail.hip")).read()
    assert text.count('"s2m2_conv_block_tail"') == 1                  # the constant; dispatch and registration both go through it
    assert "plan_dispatch_desc<s2m2_convtail_desc>(kConvTailEntry" in text and "S2M2_PLAN_DESC_ENTRY(kConvTailEntry" in text


# ---- the patch rule as a pure function

PROGRAM = r"""
#include <stdio.h>
#include "s2m2_amd/csrc/conv_select.h"
#include "s2m2_amd/csrc/convtail_select.h"
struct Layer { int N, H, W, Ho, Wo, KH, KW, Cin, Cout, stride, epi, shuffle2, korder, pool2; const float* ln_wsum; };
int main() {
    int N, H, W, C;
    while (scanf("%d %d %d %d", &N, &H, &W, &C) == 4) {
        Layer a{};
        a.N = N; a.H = a.Ho = H; a.W = a.Wo = W; a.KH = a.KW = 3; a.Cin = a.Cout = C; a.stride = 1; a.epi = S2M2_EPI_ADD; a.korder = 2;
        const s2m2::ConvChoice c = s2m2::conv_select(a, 0, true, s2m2::ConvTuning());
        const s2m2::ConvTailPatch p = s2m2::conv_tail_patch(N, H, W, C);
        printf("%d %d %d %d %d %d %d %d %d\n", N, H, W, C, p.ph, p.pw, (int)c.family, c.p[2], c.p[3]);
    }
    const int forced[][2] = {{2, 32}, {4, 32}, {4, 40}, {2, 40}, {4, 36}, {3, 32}, {0, 40}};
    for (const auto& f : forced) {
        const s2m2::ConvTailPatch p = s2m2::conv_tail_patch(1, 256, 304, 128, f[0], f[1]);
        printf("forced %d %d -> %d %d\n", f[0], f[1], p.ph, p.pw);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("convtail")
    src, exe = tmp / "patch.cpp", tmp / "patch"
    src.write_text(PROGRAM)
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", "-I", ROOT, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    # every H and W up to 320: all the sizes at which a count of 4-row, 32- or 40-column patches changes, and everything between
    text = "".join(f"{n} {h} {w} {c}\n" for n in (1, 2) for c in (128, 256) for h in range(1, 321) for w in range(1, 321))
    out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.strip().splitlines()
    rows = [tuple(int(v) for v in ln.split()) for ln in out if not ln.startswith("forced")]
    forced = dict(ln[len("forced "):].split(" -> ") for ln in out if ln.startswith("forced"))
    return rows, forced


def test_the_patch_rule_is_k5s_choice_for_the_launch_it_replaces(table):
    rows, _ = table
    assert len(rows) == 2 * 2 * 320 * 320
    frag = 4                                                          # ConvFamily::frag
    wrong = [r for r in rows if r[6] != frag or (r[4], r[5]) != (r[7], r[8])]
    assert not wrong, wrong[:10]
    chosen = {(r[3], r[4], r[5]) for r in rows}
    assert chosen == {(128, 2, 32), (128, 4, 40), (256, 2, 32), (256, 4, 40)}     # both forms are reached at both widths
    by = {(r[0], r[1], r[2], r[3]): (r[4], r[5]) for r in rows}
    assert by[(1, 256, 304, 128)] == (4, 40) and by[(2, 256, 304, 128)] == (4, 40)    # the 1/4 level of 1216 x 1024
    assert by[(1, 64, 76, 256)] == (2, 32) and by[(2, 64, 76, 256)] == (2, 32)        # the 1/16 level


def test_forced_patches(table):
    _, forced = table
    assert forced == {"2 32": "2 32", "4 32": "4 32", "4 40": "4 40", "2 40": "4 40", "4 36": "4 40", "3 32": "4 40", "0 40": "4 40"}


def test_the_header_needs_no_hip():
    text = open(os.path.join(ROOT, "s2m2_amd", "csrc", "convtail_select.h")).read()
    assert "hip/" not in text and "common.h" not in text
