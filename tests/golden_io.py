"""Golden fixtures under tests/golden are kept below 1 MiB per file.  A fixture NAME.npz that would be larger is stored as parts
NAME.part0.npz, NAME.part1.npz, ...: ordinary compressed .npz files that each hold some of its arrays.  An array too large for one part
is stored flattened, in consecutive chunks ``<key>__chunk<i>``, with its shape in ``<key>__shape``.  ``load`` rebuilds the arrays bit for
bit, from NAME.npz where that file exists and from its parts otherwise.

    python tests/golden_io.py            # split every NAME.npz above the limit into parts (after a make_golden*.py run)
"""
from __future__ import annotations

import glob
import io
import math
import os
import re
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIMIT = 1_000_000                  # bytes per file (below 1 MiB, with room for the zip directory)
_CHUNK = re.compile(r"^(.*)__chunk(\d+)$")


class Golden(dict):
    """the arrays of one fixture: a dict with the ``files`` attribute and context-manager use of ``np.load``'s NpzFile"""

    @property
    def files(self):
        return list(self.keys())

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _parts(path: str):
    stem = path[:-len(".npz")] if path.endswith(".npz") else path
    found = glob.glob(glob.escape(stem) + ".part*.npz")
    return sorted(found, key=lambda p: int(re.search(r"\.part(\d+)\.npz$", p).group(1)))


def load(name: str) -> Golden:
    """tests/golden/<name> (or an absolute path) -> {key: array}"""
    path = name if os.path.isabs(name) else os.path.join(GOLDEN, name)
    if os.path.exists(path):
        with np.load(path) as g:
            return Golden((k, g[k]) for k in g.files)
    parts = _parts(path)
    if not parts:
        raise FileNotFoundError(f"{path}: neither the file nor its parts ({os.path.basename(path)[:-4]}.partN.npz) exist")
    flat, chunks, shapes = {}, {}, {}
    for p in parts:
        with np.load(p) as g:
            for k in g.files:
                m = _CHUNK.match(k)
                if m:
                    chunks.setdefault(m.group(1), {})[int(m.group(2))] = g[k]
                elif k.endswith("__shape"):
                    shapes[k[:-len("__shape")]] = tuple(int(x) for x in g[k])
                else:
                    flat[k] = g[k]
    for k, cs in chunks.items():
        flat[k] = np.concatenate([cs[i] for i in range(len(cs))]).reshape(shapes[k])
    return Golden(flat)


def _compressed_size(arrays: dict) -> int:
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getbuffer().nbytes


def save(path: str, arrays: dict, limit: int = LIMIT) -> list:
    """write ``arrays`` as ``path`` if the compressed file fits in ``limit`` bytes, else as parts (removing ``path``) -> files written"""
    for p in _parts(path):
        os.remove(p)
    if _compressed_size(arrays) <= limit:
        np.savez_compressed(path, **arrays)
        return [path]
    entries = []                                              # (compressed size, {key: array}) units that each fit in one part
    for k, a in arrays.items():
        a = np.asarray(a)                                     # (not ascontiguousarray: that turns a 0-d array into shape (1,))
        s = _compressed_size({k: a})
        if s <= limit // 2:
            entries.append((s, {k: a}))
            continue
        n = math.ceil(s / (limit // 2))
        while True:
            pieces = np.array_split(np.ascontiguousarray(a).reshape(-1), n)
            sizes = [_compressed_size({"x": c}) for c in pieces]
            if max(sizes) <= limit // 2:
                break
            n += 1
        entries.append((64, {k + "__shape": np.asarray(a.shape, dtype=np.int64)}))
        entries += [(sz, {f"{k}__chunk{i}": c}) for i, (sz, c) in enumerate(zip(sizes, pieces))]
    bins = []                                                 # first fit, largest first
    for s, d in sorted(entries, key=lambda e: -e[0]):
        for b in bins:
            if b[0] + s <= limit * 9 // 10:
                b[0] += s
                b[1].update(d)
                break
        else:
            bins.append([s, dict(d)])
    stem = path[:-len(".npz")]
    out = []
    for i, (_, d) in enumerate(bins):
        p = f"{stem}.part{i}.npz"
        np.savez_compressed(p, **d)
        assert os.path.getsize(p) <= limit, (p, os.path.getsize(p))
        out.append(p)
    if os.path.exists(path):
        os.remove(path)
    return out


def split_all(limit: int = LIMIT) -> None:
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        if ".part" in os.path.basename(path) or os.path.getsize(path) <= limit:
            continue
        arrays = dict(load(path))
        parts = save(path, arrays, limit)
        back = load(path)
        assert back.keys() == arrays.keys() and all(back[k].dtype == a.dtype and back[k].shape == a.shape and back[k].tobytes() == a.tobytes()
                                                  for k, a in arrays.items())
        print(f"{os.path.basename(path)} -> {len(parts)} parts: " + ", ".join(f"{os.path.basename(p)} {os.path.getsize(p)}" for p in parts))


if __name__ == "__main__":
    split_all(*(int(x) for x in sys.argv[1:2]))
