"""The marching-cubes case table of K25 (``s2m2_tsdf_mesh``, include/s2m2_hip.h), generated from a construction and from nothing else.  Pure
Python, no torch, no numpy: the kernel's header (csrc/mc_table.h), the numpy oracle (tests/tsdf_mesh_oracle.py) and the tests all take the table
from ``build_table()``.  Run as a script (``python -m s2m2_amd.mc_table``) it rewrites csrc/mc_table.h.

Corner c = dx + 2 dy + 4 dz of a cell; bit c of a case is set iff the tsdf at that corner is negative.  Edge e = (axis a, base corner b with bit
a clear) joins the corners b and b | 1 << a; the edges are numbered axis-major: for a in 0..2, the bases b in ascending order.

The construction, per case:
  1. on each of the six cube faces the sign-changing edges number 0, 2 or 4.  Two are joined by a segment.  Four (the face's diagonal corners
     alike) give two segments that cut off the two NEGATIVE corners separately: each joins the two face edges that meet at a negative corner.
     A face's segments depend on its four signs alone, so the two cells that share a face agree on them.
  2. every sign-changing edge lies in two faces, so the segments close into loops; the loops are taken in the order of their lowest edge.
  3. a loop is oriented towards the positive side (free space, where K24's gradients point): with the vertices at the edge midpoints and n the
     loop's Newell normal, the sum over the loop's edges of n . (positive endpoint - negative endpoint) is > 0 (asserted non-zero).
  4. a loop is triangulated as a fan.  The apex is the first rotation of the loop, starting from its lowest edge, for which no fan diagonal lies
     in a cube face (joins two edges of one face): such a diagonal would coincide with the neighbouring cell's segment in an ambiguous face and
     leave the mesh open there.  Such an apex exists for every loop (asserted).
"""
import os

EDGES = [(a, b) for a in range(3) for b in range(8) if not b >> a & 1]         # edge number -> (axis, base corner)
EDGE_CORNERS = [(b, b | 1 << a) for a, b in EDGES]
FACES = [(f, s) for f in range(3) for s in range(2)]                           # the face of the corners with bit f == s
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mc_table.h")


def corner_xyz(c):
    return (c & 1, c >> 1 & 1, c >> 2 & 1)


def face_edges(f, s):
    """the four edge numbers whose two corners lie in face (f, s)"""
    return [e for e, (c0, c1) in enumerate(EDGE_CORNERS) if (c0 >> f & 1) == s and (c1 >> f & 1) == s]


def edges_share_a_face(e0, e1):
    return any(e0 in face_edges(f, s) and e1 in face_edges(f, s) for f, s in FACES)


def changing(case, e):
    c0, c1 = EDGE_CORNERS[e]
    return (case >> c0 & 1) != (case >> c1 & 1)


def face_segments(case, f, s):
    """step 1: the segments (unordered pairs of edge numbers) of face (f, s) under the signs of `case`"""
    fe = [e for e in face_edges(f, s) if changing(case, e)]
    if len(fe) == 0:
        return []
    if len(fe) == 2:
        return [tuple(fe)]
    assert len(fe) == 4
    segs = []
    for c in range(8):
        if (c >> f & 1) == s and case >> c & 1:                                # a negative corner of the face: the two face edges that meet at it
            pair = tuple(e for e in fe if c in EDGE_CORNERS[e])
            assert len(pair) == 2
            segs.append(pair)
    assert len(segs) == 2
    return segs


def _midpoint(e):
    p0, p1 = (corner_xyz(c) for c in EDGE_CORNERS[e])
    return tuple((x0 + x1) / 2.0 for x0, x1 in zip(p0, p1))


def _orientation(case, loop):
    """step 3's sum for the loop in the order given"""
    pts = [_midpoint(e) for e in loop]
    n = [0.0, 0.0, 0.0]
    for p, q in zip(pts, pts[1:] + pts[:1]):                                   # Newell
        n[0] += (p[1] - q[1]) * (p[2] + q[2])
        n[1] += (p[2] - q[2]) * (p[0] + q[0])
        n[2] += (p[0] - q[0]) * (p[1] + q[1])
    total = 0.0
    for e in loop:
        c0, c1 = EDGE_CORNERS[e]
        neg, pos = (c0, c1) if case >> c0 & 1 else (c1, c0)
        total += sum(nc * (xp - xn) for nc, xp, xn in zip(n, corner_xyz(pos), corner_xyz(neg)))
    return total


def case_loops(case):
    """steps 1 to 3: the oriented loops of a case, each a list of edge numbers that starts at its lowest edge, in the order of those"""
    link = {}
    for f, s in FACES:
        for e0, e1 in face_segments(case, f, s):
            link.setdefault(e0, []).append(e1)
            link.setdefault(e1, []).append(e0)
    assert all(len(v) == 2 for v in link.values()) and sorted(link) == [e for e in range(12) if changing(case, e)]
    loops, seen = [], set()
    for start in sorted(link):
        if start in seen:
            continue
        loop, prev, cur = [start], None, start
        while True:
            seen.add(cur)
            a, b = link[cur]                                                   # two different edges: two edges share at most one face
            nxt = b if a == prev else a
            if nxt == start:
                break
            assert nxt not in seen
            loop.append(nxt)
            prev, cur = cur, nxt
        assert len(loop) >= 3
        o = _orientation(case, loop)
        assert o != 0.0
        if o < 0:
            loop = loop[:1] + loop[:0:-1]
        loops.append(loop)
    return loops


def fan(loop):
    """step 4: the triangles of one oriented loop"""
    n = len(loop)
    for r in range(n):
        rot = loop[r:] + loop[:r]
        if not any(edges_share_a_face(rot[0], rot[i]) for i in range(2, n - 1)):
            return [(rot[0], rot[i], rot[i + 1]) for i in range(1, n - 1)]
    raise AssertionError(f"no apex for the loop {loop}")


def build_table():
    """-> list of 256 lists of triangles, a triangle a tuple of three edge numbers"""
    return [[tri for loop in case_loops(case) for tri in fan(loop)] for case in range(256)]


def max_triangles(table):
    return max(len(t) for t in table)


def header_text(table=None):
    """the text of csrc/mc_table.h: one row per case, its number of triangles followed by their edge numbers, padded with zeros"""
    table = build_table() if table is None else table
    most = max_triangles(table)
    assert most == 5, "the kernels' 16-byte rows (one count and 3 * 5 edge numbers) hold at most 5 triangles per case"
    row = 1 + 3 * most
    lines = ["// GENERATED by s2m2_amd/mc_table.py (python -m s2m2_amd.mc_table) -- do not edit; tests/test_tsdf_mesh_cpu.py compares the bytes.",
             "// K25's marching-cubes case table: row = case (bit c set iff the tsdf at corner c = dx + 2 dy + 4 dz is negative); byte 0 the number of",
             "// triangles, then three edge numbers per triangle; edge = (axis a, base corner b with bit a clear), numbered axis-major.",
             "#pragma once",
             "",
             "namespace s2m2 {",
             "",
             f"constexpr int kMcMaxTriangles = {most};",
             f"constexpr int kMcRowBytes = {row};",
             "",
             "alignas(16) __constant__ const unsigned char kMcTable[256][kMcRowBytes] = {"]
    for case, tris in enumerate(table):
        flat = [len(tris)] + [e for tri in tris for e in tri]
        flat += [0] * (row - len(flat))
        lines.append("    {" + ", ".join(f"{x:2d}" for x in flat) + "},  // " + f"{case:3d}")
    lines += ["};", "", "}  // namespace s2m2", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    with open(HEADER, "w") as f:
        f.write(header_text())
    print(HEADER)
