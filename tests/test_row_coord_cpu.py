"""s2m2_amd/csrc/row_coord.h on the CPU: the header is plain C++ (no HIP), so a small host program compiled from it checks the 32-bit row ->
(n, y, x) decomposition and the division-free walk (RowWalk<K>::step) against plain 64-bit division:
  * every row of every (N, Ho, Wo) grid with Ho, Wo in {1, 2, 3, 5, 38, 76, 304} and N in {1, 2, 3};
  * every row distance the kernels use between a thread's pieces (4, 8, 16, 32, 64), from every row, also past the last row of the grid (the
    ragged last tile walks on into images that do not exist) and where Wo is smaller than the distance;
  * rows at and around 2^31 - 1 (every entry point requires rows < 2^31; a tile may reach a little past it).
The same program is built a second time with -fsanitize=address,undefined as a stand-alone binary and must run clean."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdio.h>
#include "s2m2_amd/csrc/row_coord.h"

static long long bad = 0, checked = 0;

static void expect(long long m, unsigned Ho, unsigned Wo, const s2m2::RowCoord& c, const char* what, unsigned K) {
    const long long x = m % Wo, t = m / Wo, y = t % Ho, n = t / Ho;            // the reference: 64-bit division
    ++checked;
    if ((long long)c.n != n || (long long)c.y != y || (long long)c.x != x) {
        if (bad++ < 20) printf("MISMATCH %s K=%u m=%lld Ho=%u Wo=%u: got (%u, %u, %u), want (%lld, %lld, %lld)\n", what, K, m, Ho, Wo, c.n, c.y, c.x, n, y, x);
    }
}

template <unsigned K>
static void walk_from(long long m, unsigned Ho, unsigned Wo) {
    const s2m2::RowWalk<K> w(Ho, Wo);
    s2m2::RowCoord c = w.decompose((unsigned)m);
    expect(m, Ho, Wo, c, "decompose", K);
    w.step(c);
    expect(m + K, Ho, Wo, c, "step", K);
}

// a thread's whole walk: 8 pieces from one decomposition
template <unsigned K>
static void long_walk(long long m, unsigned Ho, unsigned Wo) {
    const s2m2::RowWalk<K> w(Ho, Wo);
    s2m2::RowCoord c = w.decompose((unsigned)m);
    for (int it = 1; it <= 8; ++it) {
        w.step(c);
        expect(m + (long long)it * K, Ho, Wo, c, "walk", K);
    }
}

static void all_steps(long long m, unsigned Ho, unsigned Wo) {
    walk_from<4>(m, Ho, Wo);
    walk_from<8>(m, Ho, Wo);
    walk_from<16>(m, Ho, Wo);
    walk_from<32>(m, Ho, Wo);
    walk_from<64>(m, Ho, Wo);
}

int main() {
    static const unsigned dims[] = {1, 2, 3, 5, 38, 76, 304};
    for (unsigned Ho : dims)
        for (unsigned Wo : dims) {
            for (unsigned N = 1; N <= 3; ++N) {
                const long long rows = (long long)N * Ho * Wo;
                for (long long m = 0; m < rows; ++m) all_steps(m, Ho, Wo);
                for (long long m = 0; m < rows; m += 7) { long_walk<16>(m, Ho, Wo); long_walk<64>(m, Ho, Wo); long_walk<4>(m, Ho, Wo); }
            }
            const long long top = (1LL << 31) - 1;
            for (long long m = top - 400; m <= top + 128; ++m) { all_steps(m, Ho, Wo); long_walk<64>(m, Ho, Wo); }
        }
    // the extent check of the host entry points
    if (!s2m2::image_extent_fits_u32(304 * 256, 128) || s2m2::image_extent_fits_u32(1LL << 20, 1LL << 12) || !s2m2::image_extent_fits_u32((1LL << 20) - 1, 1LL << 12)
        || s2m2::image_extent_fits_u32(0, 8)) {
        printf("MISMATCH image_extent_fits_u32\n");
        ++bad;
    }
    printf("checked %lld bad %lld\n", checked, bad);
    return bad ? 1 : 0;
}
"""


def _compiler():
    for cc in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cc)
        if path:
            return path
    raise RuntimeError("no host C++ compiler found (c++, g++, clang++)")


@pytest.fixture(scope="module")
def source(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("row_coord")
    src = tmp / "row_coord.cpp"
    src.write_text(PROGRAM)
    return tmp, src


def _build_and_run(tmp, src, name, flags):
    exe = tmp / name
    subprocess.run([_compiler(), "-std=c++17", "-Wall", *flags, "-I", ROOT, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_header_needs_no_hip():
    text = open(os.path.join(ROOT, "s2m2_amd", "csrc", "row_coord.h")).read()
    assert "hip/" not in text and "common.h" not in text


def test_decompose_and_step_equal_64_bit_division(source):
    r = _build_and_run(*source, "row_coord", ["-O2"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "checked" and int(last[1]) > 5_000_000 and int(last[3]) == 0


def test_same_program_under_address_and_undefined_sanitizers(source):
    """stand-alone binary, sanitizer runtimes linked in: unsigned wrap is defined, so any report is a real fault in the header or the program"""
    r = _build_and_run(*source, "row_coord_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1].endswith("bad 0")
