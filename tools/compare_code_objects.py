#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libs2m2_hip.so, kernel by kernel (no GPU needed).

    python tools/compare_code_objects.py OLD.so NEW.so

Unbundles every gfx950 code object of both libraries and compares, per kernel symbol, the instruction bytes and the kernel descriptor (VGPR /
SGPR / LDS / scratch words; the descriptor's entry offset is masked: it is the distance to the code, which moves with the order of the
instantiations in a translation unit).  Exit status 0 only if both libraries hold the same set of kernels and every kernel is identical --
the argument of a host-only refactor that numerics and kernel times cannot have moved."""
import struct
import subprocess
import sys

READELF = "/opt/rocm/llvm/bin/llvm-readelf"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib):
    data = open(lib, "rb").read()
    pos = data.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", data, p)
            ident = data[p + 24:p + 24 + idlen].decode()
            p += 24 + idlen
            if "gfx950" in ident and size:
                yield data[pos + off:pos + off + size]
        pos = data.find(MAGIC, pos + len(MAGIC))


def kernels(elf, tmp):
    """{kernel name: (code bytes, descriptor bytes with the entry offset masked)}"""
    open(tmp, "wb").write(elf)
    secs = {}
    for line in subprocess.run([READELF, "-S", "-W", tmp], capture_output=True, text=True, check=True).stdout.splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) >= 6 and f[0].isdigit():
            secs[int(f[0])] = (int(f[3], 16), int(f[4], 16))        # address, file offset
    syms = {}
    for line in subprocess.run([READELF, "-s", "-W", tmp], capture_output=True, text=True, check=True).stdout.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
            addr, off = secs[int(f[6])]
            start = int(f[1], 16) - addr + off
            syms[f[7]] = elf[start:start + int(f[2])]
    out = {}
    for name, kd in syms.items():
        if name.endswith(".kd") and name[:-3] in syms:
            out[name[:-3]] = (syms[name[:-3]], kd[:16] + bytes(8) + kd[24:])
    return out


def all_kernels(lib):
    out = {}
    for i, elf in enumerate(code_objects(lib)):
        for name, v in kernels(elf, f"/tmp/compare_code_objects.{i}.elf").items():
            assert name not in out or out[name] == v, f"{lib}: two different copies of {name}"
            out[name] = v
    return out


def main():
    old, new = all_kernels(sys.argv[1]), all_kernels(sys.argv[2])
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    code = [k for k in old if k in new and old[k][0] != new[k][0]]
    desc = [k for k in old if k in new and old[k][1] != new[k][1]]
    for title, names in (("only in OLD", gone), ("only in NEW", added), ("code differs", code), ("descriptor differs", desc)):
        for k in names:
            print(f"{title}: {k}")
    print(f"kernels: {len(old)} old, {len(new)} new; {len(gone)} removed, {len(added)} added, {len(code)} with different code, "
          f"{len(desc)} with different descriptors; {sum(len(v[0]) for v in new.values())} code bytes compared")
    return 1 if gone or added or code or desc else 0


if __name__ == "__main__":
    sys.exit(main())
