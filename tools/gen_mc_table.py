"""Generates the marching-cubes case table of sph_extract_surface (include/sphmi.h) and writes it as
smoothed-particle-hydrodynamics_amd/csrc/sph_mc_table.h. The generated header is committed; tests/test_surface_host.py checks
that it equals this script's output, and tests/surface_ref.py imports TABLE from here.

The table follows from four rules rather than being typed in:
  1. On each cube face, join crossed edges with segments: two crossed edges give one segment; four crossed edges (two inside
     corners on a diagonal) cut each inside corner off on its own. The rule reads only the face's corners, so two cells that
     share a face put the same segments on it (a watertight mesh).
  2. Each segment is directed so that, seen from outside the cube, the inside side of the face lies to its right.
  3. The directed segments form disjoint cycles; each starts at its smallest edge, cycles in ascending order of that edge.
  4. A cycle c0..c(L-1) is cut into the fan (c0, cq, c(q+1)), q = 1..L-2, of its first rotation whose chords (c0, cq),
     q = 2..L-2, never join two edges of a common cube face (a chord on a face could meet the neighbour cell's chord there).
Triangles wound this way have normals (v1-v0)x(v2-v0) that point from inside to outside.

    python tools/gen_mc_table.py [--check]   (--check: exit 1 if the committed header differs)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "smoothed-particle-hydrodynamics_amd", "csrc", "sph_mc_table.h")

# corner c sits at (c & 1, (c >> 1) & 1, c >> 2)
CORNERS = [(c & 1, (c >> 1) & 1, c >> 2) for c in range(8)]
# edges 0..3 along x, 4..7 along y, 8..11 along z; edge e starts at its first corner and has axis e // 4
EDGES = [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7)]
MAX_TRIS = 5


def _faces():
    """(corners in cyclic order around the face, outward normal) for the six faces."""
    faces = []
    for axis in range(3):
        for side in (0, 1):
            ring = [c for c in range(8) if CORNERS[c][axis] == side]
            # cyclic order: the two other axes' bits walk (0,0) (1,0) (1,1) (0,1)
            u, v = [a for a in range(3) if a != axis]
            ring.sort(key=lambda c: [(0, 0), (1, 0), (1, 1), (0, 1)].index((CORNERS[c][u], CORNERS[c][v])))
            n = [0, 0, 0]
            n[axis] = 1 if side else -1
            faces.append((ring, tuple(n)))
    return faces


FACES = _faces()


def _edge_of(a, b):
    return EDGES.index((min(a, b), max(a, b)))


FACE_EDGES = [set(_edge_of(r[q], r[(q + 1) % 4]) for q in range(4)) for r, _ in FACES]


def _mid(e):
    a, b = EDGES[e]
    return tuple((CORNERS[a][k] + CORNERS[b][k]) / 2.0 for k in range(3))


def _sub(p, q):
    return tuple(p[k] - q[k] for k in range(3))


def _cross(p, q):
    return (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])


def _dot(p, q):
    return sum(p[k] * q[k] for k in range(3))


def _directed(a, b, corner, n):
    """Segment between edges a and b directed so that `corner` (an inside corner it cuts off, or on the inside side of it) lies
    to the right of its direction seen from outside the face (right = direction x outward normal)."""
    d = _sub(_mid(b), _mid(a))
    s = _dot(_sub(CORNERS[corner], _mid(a)), _cross(d, n))
    assert s != 0
    return (a, b) if s > 0 else (b, a)


def face_segments(case):
    """Rules 1 and 2: the directed segments (from edge, to edge) of every face of `case`."""
    inside = [(case >> c) & 1 for c in range(8)]
    segs = []
    for ring, n in FACES:
        crossed = [q for q in range(4) if inside[ring[q]] != inside[ring[(q + 1) % 4]]]
        if not crossed:
            continue
        if len(crossed) == 2:
            a, b = (_edge_of(ring[q], ring[(q + 1) % 4]) for q in crossed)
            corner = next(c for c in ring if inside[c])
            segs.append(_directed(a, b, corner, n))
        else:  # 4: two inside corners on a diagonal, each cut off on its own
            for q in range(4):
                c = ring[q]
                if inside[c]:
                    a = _edge_of(ring[(q - 1) % 4], c)
                    b = _edge_of(c, ring[(q + 1) % 4])
                    segs.append(_directed(a, b, c, n))
    return segs


def cycles(case):
    """Rule 3: the cycles of the directed segments, each from its smallest edge, in ascending order of it."""
    nxt = {}
    for a, b in face_segments(case):
        assert a not in nxt, "edge %d leaves twice in case %d" % (a, case)
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), "open segment chain in case %d" % case
    out, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        cyc = [e]
        seen.add(e)
        while nxt[cyc[-1]] != e:
            cyc.append(nxt[cyc[-1]])
            seen.add(cyc[-1])
        out.append(cyc)
    return out


def _share_face(a, b):
    return any(a in f and b in f for f in FACE_EDGES)


def fan(cyc):
    """Rule 4: the fan of the first rotation with no chord on a cube face."""
    L = len(cyc)
    for r in range(L):
        c = cyc[r:] + cyc[:r]
        if all(not _share_face(c[0], c[q]) for q in range(2, L - 1)):
            return [(c[0], c[q], c[q + 1]) for q in range(1, L - 1)]
    raise AssertionError("no admissible fan for cycle %r" % (cyc,))


def case_triangles(case):
    return [t for cyc in cycles(case) for t in fan(cyc)]


TABLE = [case_triangles(c) for c in range(256)]


def render():
    lines = ["// Generated by tools/gen_mc_table.py -- do not edit. Marching-cubes case table of sph_extract_surface",
             "// (include/sphmi.h, DESIGN.md §13): case = sum of inside(corner c) << c; each triangle is three cube edges",
             "// (0..3 along x, 4..7 along y, 8..11 along z), wound so that (v1-v0)x(v2-v0) points from inside to outside.",
             "#pragma once",
             "",
             "// sph_surface.hip defines this as `static __constant__ const` (device constant memory)",
             "#ifndef SPH_MC_TABLE_QUALIFIER",
             "#define SPH_MC_TABLE_QUALIFIER static const",
             "#endif",
             "",
             "#define SPH_MC_MAX_TRIS %d" % MAX_TRIS,
             "",
             "// triangles per case",
             "SPH_MC_TABLE_QUALIFIER unsigned char kMcTriCount[256] = {"]
    counts = [len(t) for t in TABLE]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(v) for v in counts[r:r + 32]) + ",")
    lines.append("};")
    lines.append("")
    lines.append("// edges of each case's triangles, 3 per triangle, unused entries 0")
    lines.append("SPH_MC_TABLE_QUALIFIER unsigned char kMcTriEdges[256][3 * SPH_MC_MAX_TRIS] = {")
    for c in range(256):
        flat = [e for t in TABLE[c] for e in t]
        flat += [0] * (3 * MAX_TRIS - len(flat))
        lines.append("    {" + ", ".join(str(v) for v in flat) + "},  // %d" % c)
    lines.append("};")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv[1:]:
        with open(HEADER) as f:
            sys.exit(0 if f.read() == text else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote %s: %d triangles over 256 cases" % (HEADER, sum(len(t) for t in TABLE)))
