#!/usr/bin/env python3
"""Writes mc_table.h, the marching-cubes case table of csrc/mesh.hip (include/nerf_hip.h "mesh extraction"), from one rule:

    python gen_mc_table.py > mc_table.h        (the Makefile does not run it; tests/test_mesh_host.py checks the output)

Corner c in [0, 8) of a cell sits at (c & 1, (c >> 1) & 1, c >> 2).  Edge e joins corner EDGE_CORNER[e] to that corner + e_a,
a = EDGE_AXIS[e]; the edges are numbered by (corner, axis), so edge e is owned by the lattice point at corner EDGE_CORNER[e].

  * Face rule: on each of the 6 cube faces the crossing edges (one end inside, one outside) are joined in pairs.  With two
    crossing edges they form one segment.  With four (the inside corners are the two ends of a diagonal) the inside corners are
    kept apart: each inside corner's two edges on that face form a segment.  The rule reads the face's four corners only, so
    two cells agree on every face they share.
  * Every crossing edge lies on two faces and has one segment on each: the segments form disjoint loops, one polygon each.
    A loop is oriented so that its triangles' normals (b - a) x (c - a) point from the inside (v > iso) to the outside, and
    starts at its smallest edge; loops are emitted in the order of their smallest edges.
  * A loop is fan-triangulated from its first vertex, in loop order, whose fan diagonals never join two edges that lie on a
    common cube face (such a diagonal could be emitted by the neighbour across that face too, and the mesh would not be a
    manifold there).  The generator asserts that such an apex exists for every loop.

Table row of case s = sum(inside(c) << c): [triangle count, then 3 edge ids per triangle, zero padded to MAX_TRIS triangles].
"""
import sys

EDGES = [(c, a) for c in range(8) for a in range(3) if not (c >> a) & 1]          # (corner, axis), by owner then axis
EDGE_CORNER = [c for c, _ in EDGES]
EDGE_AXIS = [a for _, a in EDGES]
MAX_TRIS = 5                 # asserted below: the largest triangle count of any case
TOTAL_TRIS = 820             # asserted below: triangles over the 256 cases


def corner_pos(c):
    return (c & 1, (c >> 1) & 1, c >> 2)


def edge_ends(e):
    c, a = EDGES[e]
    return c, c | (1 << a)


def edge_mid(e):
    p, q = (corner_pos(x) for x in edge_ends(e))
    return tuple(0.5 * (u + v) for u, v in zip(p, q))


def faces():
    """(axis, side, corners, edges) of the 6 faces; outward normal (2 side - 1) e_axis."""
    out = []
    for a in range(3):
        for s in (0, 1):
            cs = [c for c in range(8) if ((c >> a) & 1) == s]
            es = [e for e, (c, b) in enumerate(EDGES) if b != a and ((c >> a) & 1) == s]
            out.append((a, s, cs, es))
    return out


FACES = faces()
EDGE_FACES = [frozenset(f for f, (_, _, _, es) in enumerate(FACES) if e in es) for e in range(12)]


def _sub(p, q):
    return tuple(u - v for u, v in zip(p, q))


def _cross(p, q):
    return (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])


def _dot(p, q):
    return sum(u * v for u, v in zip(p, q))


def face_segments(case, f):
    """Segments (e0, e1, m) of face f: m is an in-face direction from the inside corners of the segment to the outside."""
    a, s, cs, es = FACES[f]
    inside = [c for c in cs if (case >> c) & 1]
    cross = [e for e in es if ((case >> edge_ends(e)[0]) & 1) != ((case >> edge_ends(e)[1]) & 1)]
    if not cross:
        return []
    if len(cross) == 2:
        outside = [c for c in cs if c not in inside]
        mi = [sum(corner_pos(c)[k] for c in inside) / len(inside) for k in range(3)]
        mo = [sum(corner_pos(c)[k] for c in outside) / len(outside) for k in range(3)]
        return [(cross[0], cross[1], _sub(mo, mi))]
    assert len(cross) == 4 and len(inside) == 2
    segs = []
    for c in inside:                                          # the ambiguous face: each inside corner keeps its own segment
        ec = [e for e in cross if c in edge_ends(e)]
        assert len(ec) == 2
        mid = tuple(0.5 * (u + v) for u, v in zip(edge_mid(ec[0]), edge_mid(ec[1])))
        segs.append((ec[0], ec[1], _sub(mid, corner_pos(c))))
    return segs


def case_loops(case):
    """The oriented loops of a case (lists of edge ids), in the order of their smallest edges, each starting there."""
    nxt = {}                                                  # directed: e -> the next edge of its loop
    for f in range(6):
        a, s, _, _ = FACES[f]
        n_f = tuple((2 * s - 1) if k == a else 0 for k in range(3))
        for e0, e1, m in face_segments(case, f):
            t = _cross(m, n_f)                                # boundary direction of a surface whose normal is m (see below)
            d = _dot(_sub(edge_mid(e1), edge_mid(e0)), t)
            assert d != 0
            p, q = (e0, e1) if d > 0 else (e1, e0)
            assert p not in nxt
            nxt[p] = q
    # the surface's normal m points to the outside and the surface lies on the cube's side (-n_f) of its boundary on a face:
    # traversing the boundary along m x n_f keeps the surface on the left seen from +m (m x (m x n_f) = -n_f), so the loops
    # carry the counter-clockwise orientation of their polygons seen from the outside
    assert sorted(nxt) == sorted(nxt.values())
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop = [e]
        seen.add(e)
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
            seen.add(loop[-1])
        loops.append(loop)
    return loops


def fan(loop):
    """Triangles of one loop: a fan from the first apex whose diagonals join no two edges of a common face."""
    L = len(loop)
    for s in range(L):
        v = loop[s:] + loop[:s]
        if all(not (EDGE_FACES[v[0]] & EDGE_FACES[v[i]]) for i in range(2, L - 1)):
            return [(v[0], v[i], v[i + 1]) for i in range(1, L - 1)]
    raise AssertionError(f"no apex for loop {loop}")


def case_triangles(case):
    return [t for loop in case_loops(case) for t in fan(loop)]


def table():
    rows = [case_triangles(s) for s in range(256)]
    assert max(len(r) for r in rows) == MAX_TRIS, max(len(r) for r in rows)
    assert sum(len(r) for r in rows) == TOTAL_TRIS, sum(len(r) for r in rows)
    return rows


def header():
    rows = table()
    out = ["/* mc_table.h -- generated by gen_mc_table.py (do not edit): the marching-cubes case table of mesh.hip.",
           " * Row s (s = sum of inside(c) << c over the corners c of a cell): triangle count, then 3 edge ids per triangle,",
           f" * zero padded to NERF_MC_MAX_TRIS.  Edge e joins corner NERF_MC_EDGE_CORNER[e] to that corner + e_(NERF_MC_EDGE_AXIS[e]). */",
           "#ifndef NERF_MC_TABLE_H", "#define NERF_MC_TABLE_H", "",
           f"#define NERF_MC_MAX_TRIS {MAX_TRIS}",
           "#define NERF_MC_ROW (1 + 3 * NERF_MC_MAX_TRIS)",
           "#define NERF_MC_EDGE_CORNER_INIT {" + ", ".join(map(str, EDGE_CORNER)) + "}",
           "#define NERF_MC_EDGE_AXIS_INIT {" + ", ".join(map(str, EDGE_AXIS)) + "}",
           "#define NERF_MC_TABLE_INIT { \\"]
    for s, r in enumerate(rows):
        vals = [len(r)] + [e for t in r for e in t]
        vals += [0] * (1 + 3 * MAX_TRIS - len(vals))
        out.append("  {" + ", ".join(f"{x:2d}" for x in vals) + "}" + ("," if s < 255 else "") + f"  /* {s:3d} */ \\")
    out += ["}", "", "#endif /* NERF_MC_TABLE_H */", ""]
    return "\n".join(out)


if __name__ == "__main__":
    sys.stdout.write(header())
