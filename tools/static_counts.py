#!/usr/bin/env python3
"""Static instruction counts per kernel of a .hip source (or of gfx950 assembly already emitted with -S), no GPU: total instructions and
the classes that say where a kernel's issue slots go -- vector ALU, scalar ALU, MFMA, 64-bit index arithmetic (s_mul_*, s_addc / v_addc),
branches, s_nop, v_accvgpr moves, global loads / stores, LDS accesses.  Registers and spills: tools/kernel_resources.py, tools/isa_audit.py.

    python tools/static_counts.py s2m2_amd/csrc/fusion.hip [substring of the demangled kernel name ...]
    python tools/static_counts.py fusion.s feature_fusion_direct
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on", "-fno-fast-math", "--cuda-device-only", "-S",
         "-I" + os.path.join(ROOT, "include")]
CLASSES = [("mfma", r"v_mfma"), ("accvgpr", r"v_accvgpr"), ("s_nop", r"s_nop"), ("s_mul", r"s_mul_"), ("addc", r"[sv]_addc"),
           ("branch", r"s_cbranch|s_branch"), ("gload", r"global_load"), ("gstore", r"global_store"), ("lds", r"ds_"),
           ("waitcnt", r"s_waitcnt"), ("barrier", r"s_barrier")]


def counts(text):
    out, cur = {}, None
    for line in text.splitlines():
        if line.startswith("_Z") and "; @_Z" in line:
            cur = line.split(":")[0]
            out[cur] = dict(total=0, valu=0, salu=0, **{k: 0 for k, _ in CLASSES})
            continue
        if cur is None:
            continue
        m = re.match(r"\s+([a-z][a-z0-9_]+)\b", line)
        if not m:
            continue
        op, c = m.group(1), out[cur]
        c["total"] += 1
        hit = False
        for k, pat in CLASSES:
            if re.match(pat, op):
                c[k] += 1
                hit = True
        if op.startswith("v_") and not op.startswith(("v_mfma", "v_accvgpr")):
            c["valu"] += 1
        elif op.startswith("s_") and not hit and "load" not in op and not op.startswith(("s_endpgm", "s_set", "s_sleep")):
            c["salu"] += 1
        if op == "s_endpgm":
            cur = None
    return out


def main():
    src, subs = sys.argv[1], sys.argv[2:]
    if src.endswith(".s"):
        text = open(src).read()
    else:
        with tempfile.TemporaryDirectory() as td:
            asm = os.path.join(td, "a.s")
            r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *os.environ.get("S2M2_BUILD_DEFINES", "").split(), src, "-o", asm], capture_output=True, text=True)
            if r.returncode:
                sys.exit(r.stderr[-3000:])
            text = open(asm).read()
    keys = ["total", "valu", "salu"] + [k for k, _ in CLASSES]
    print(" ".join(f"{k:>7}" for k in keys) + "  kernel")
    for name, c in counts(text).items():
        dm = subprocess.run(["c++filt", "-p", name], capture_output=True, text=True).stdout.strip() or name
        dm = re.sub(r"^void s2m2::", "", dm)
        if subs and not any(s in dm for s in subs):
            continue
        print(" ".join(f"{c[k]:7d}" for k in keys) + "  " + dm[:140])


if __name__ == "__main__":
    main()
