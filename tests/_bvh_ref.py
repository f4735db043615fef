"""numpy reference of include/nerf_hip.h "mesh BVH" (a helper module, not a test): the Morton keys, the sorted order, the node boxes
in heap order, the stackless traversal with its pruning rule -- emulated point by point, counting the leaves it enters and the faces
it tests -- and the closest point of a given face.  Validity, the region tests' arithmetic and the brute force are
tests/_distance_ref.py's."""
import numpy as np

from tests import _distance_ref as D

F32 = np.float32
LEAF, CELLS, KEY_SHIFT, INVALID_CODE = 4, 4096, 24, 1 << 36
NAN32 = np.array([D.NAN_BITS], np.uint32).view(F32)[0]
NONE = (0x7F800000 << 32) | 0xFFFFFFFF


def tree_shape(F):
    """(nL, P, depth, launches): ceil(F / 4) leaves, P the smallest power of two >= max(nL, 1), depth = log2 P, and the launches of
    the build: the leaves, one per level above the levels 8 .. 0, and those in one."""
    nL = -(-F // LEAF)
    P = 1
    while P < nL:
        P *= 2
    depth = P.bit_length() - 1
    return nL, P, depth, 2 + max(0, depth - 9)


def morton(cells):
    """int64 code of int cells [..., 3] in [0, 4096): bit 3 i + a of the code is bit i of axis a (the plain loop)."""
    c = np.asarray(cells, np.int64)
    code = np.zeros(c.shape[:-1], np.int64)
    for i in range(12):
        for a in range(3):
            code |= ((c[..., a] >> i) & 1) << (3 * i + a)
    return code


def cells_of(m, lo, hi):
    """The Morton cell per axis of float64 coordinates m [..., 3]: clamp(floor((m - lo) / ext * 4096), 0, 4095)."""
    lo64, hi64 = np.asarray(lo, F32).astype(np.float64), np.asarray(hi, F32).astype(np.float64)
    t = (np.asarray(m, np.float64) - lo64) / (hi64 - lo64) * float(CELLS)
    return np.clip(np.floor(t), 0, CELLS - 1).astype(np.int64)


def keys(verts, faces, lo, hi):
    """int64 [F]: code 2^24 + f, the code of the bounding-box midpoint (float64) for a valid face and 2^36 for any other."""
    ok, a, b, c, _ = D.corners(verts, faces)
    F = len(ok)
    mn = np.minimum(np.minimum(a, b), c).astype(np.float64)
    mx = np.maximum(np.maximum(a, b), c).astype(np.float64)
    code = morton(cells_of((mn + mx) * 0.5, lo, hi)) if F else np.zeros(0, np.int64)
    code = np.where(ok, code, INVALID_CODE)
    return code * (1 << KEY_SHIFT) + np.arange(F, dtype=np.int64)


def order(verts, faces, lo, hi):
    """int32 [F]: the face of each key in ascending order, -1 for an invalid face (they sort behind every valid one)."""
    k = np.sort(keys(verts, faces, lo, hi))
    f = (k & ((1 << KEY_SHIFT) - 1)).astype(np.int32)
    return np.where((k >> KEY_SHIFT) < INVALID_CODE, f, -1).astype(np.int32)


def nodes(verts, faces, lo, hi):
    """float32 [2 P, 6]: (min x y z, max x y z) per node in heap order, (+inf, -inf) for a node without a valid face and for the
    unused node 0."""
    ok, a, b, c, _ = D.corners(verts, faces)
    o = order(verts, faces, lo, hi)
    _, P, _, _ = tree_shape(len(o))
    out = np.empty((2 * P, 6), F32)
    out[:, :3], out[:, 3:] = np.inf, -np.inf
    for s, f in enumerate(o):
        if f < 0:
            continue
        i = P + s // LEAF
        corner = np.stack([a[f], b[f], c[f]])
        out[i, :3] = np.minimum(out[i, :3], corner.min(0))
        out[i, 3:] = np.maximum(out[i, 3:], corner.max(0))
    for i in range(P - 1, 0, -1):
        out[i, :3] = np.minimum(out[2 * i, :3], out[2 * i + 1, :3])
        out[i, 3:] = np.maximum(out[2 * i, 3:], out[2 * i + 1, 3:])
    return out


def _box_d2(p64, node):
    if node[0] > node[3]:
        return np.inf
    d = np.maximum(np.maximum(node[:3].astype(np.float64) - p64, p64 - node[3:].astype(np.float64)), 0.0)
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def _skip(m2, slack, best):
    """The rule: skipped only if empty, or m > slack and (m - slack)^2 (1 - 2^-20) > the best D, strictly."""
    if m2 == np.inf:
        return True
    Dbest = float(np.array([best >> 32], np.uint32).view(F32)[0])
    s = np.sqrt(m2) - slack
    return bool(s > 0.0 and (s * s) * (1.0 - 2.0 ** -20) > Dbest)


class Tree:
    """The hierarchy of one mesh, built once; query() walks it for every point."""

    def __init__(self, verts, faces, lo=D.LO, hi=D.HI):
        self.ok, self.a, self.b, self.c, _ = D.corners(verts, faces)
        self.F = len(self.ok)
        self.order = order(verts, faces, lo, hi)
        self.nodes = nodes(verts, faces, lo, hi)
        self.nL, self.P, self.depth, self.launches = tree_shape(self.F)
        self.box_abs = F32(max(np.abs(np.asarray(lo, F32)).max(), np.abs(np.asarray(hi, F32)).max()))

    def one(self, p):
        """(key of the answer, leaves entered, faces tested) for one finite float32 point: the kernel's walk, step for step."""
        p = np.asarray(p, F32)
        root = self.nodes[1]
        best, leaves, cands = NONE, 0, 0
        if not root[0] <= root[3]:
            return best, leaves, cands
        S = F32(max(np.abs(p).max(), np.abs(root).max(), self.box_abs))
        slack = float(S) * 2.0 ** -18
        p64 = p.astype(np.float64)
        node, trail, P = 1, 0, self.P
        while True:
            up = False
            if node >= P:
                leaves += 1
                s0 = LEAF * (node - P)
                for s in range(s0, min(s0 + LEAF, self.F)):
                    f = int(self.order[s])
                    if f < 0:
                        continue
                    cands += 1
                    d = D.point_triangle_d2(p, self.a[f], self.b[f], self.c[f])
                    if not np.isnan(d):
                        best = min(best, (int(np.array([d], F32).view(np.uint32)[0]) << 32) | f)
                up = True
            else:
                ml, mr = _box_d2(p64, self.nodes[2 * node]), _box_d2(p64, self.nodes[2 * node + 1])
                right = mr < ml
                near_ok = not _skip(mr if right else ml, slack, best)
                far_ok = not _skip(ml if right else mr, slack, best)
                nearer = 2 * node + int(right)
                if near_ok:
                    node, trail = nearer, ((trail << 1) | int(far_ok)) & 0xFFFFFFFF
                elif far_ok:
                    node, trail = nearer ^ 1, (trail << 1) & 0xFFFFFFFF
                else:
                    up = True
            if not up:
                continue
            done = False
            while True:
                if trail == 0:
                    done = True
                    break
                k = (trail & -trail).bit_length() - 1
                trail = (trail >> k) & ~1
                node = (node >> k) ^ 1
                if not _skip(_box_d2(p64, self.nodes[node]), slack, best):
                    break
            if done:
                break
        return best, leaves, cands

    def query(self, points):
        """(dist2 [n] float32, face [n] int32, leaves entered [n], faces tested [n])."""
        pts = np.asarray(points, F32).reshape(-1, 3)
        n = len(pts)
        bits, face = np.full(n, D.NAN_BITS, np.uint32), np.full(n, -1, np.int32)
        leaves, cands = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for i in np.nonzero(np.isfinite(pts).all(1))[0]:
            best, leaves[i], cands[i] = self.one(pts[i])
            bits[i] = best >> 32
            face[i] = np.array([best & 0xFFFFFFFF], np.uint32).view(np.int32)[0]
        return bits.view(F32), face, leaves, cands


def closest(points, verts, faces, face):
    """float32 [n, 3]: the q of the region tests for point i and face[i] (D.point_triangle_d2's arithmetic, operator for operator,
    with q returned); NaN for a face of -1, out of range or invalid."""
    pts = np.asarray(points, F32).reshape(-1, 3)
    face = np.asarray(face, np.int64)
    ok, A, B, C, _ = D.corners(verts, faces)
    F = len(ok)
    good = (face >= 0) & (face < F)
    g = np.where(good, face, 0)
    out = np.full((len(pts), 3), NAN32, F32)
    if F == 0 or not len(pts):
        return out
    good &= ok[g]
    p, a, b, c = pts, A[g], B[g], C[g]
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp, bc = b - a, c - a, p - a, p - b, p - c, c - b
        d1, d2, d3, d4, d5, d6 = D._dot(ab, ap), D._dot(ac, ap), D._dot(ab, bp), D._dot(ac, bp), D._dot(ab, cp), D._dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        s = (va + vb) + vc
        q = (a + D._div(vb, s)[..., None] * ab) + D._div(vc, s)[..., None] * ac
        tests = [(va <= 0) & (e43 >= 0) & (e56 >= 0), (vb <= 0) & (d2 >= 0) & (d6 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d3 >= 0) & (d4 <= d3), (d1 <= 0) & (d2 <= 0)]
        cand = [b + D._div(e43, e43 + e56)[..., None] * bc, a + D._div(d2, d2 - d6)[..., None] * ac, c,
                a + D._div(d1, d1 - d3)[..., None] * ab, b, a]
        for t, x in zip(tests, cand):                                  # the last assignment wins: the header's first test
            q = np.where(t[..., None], x, q)
    return np.where(good[:, None], q.astype(F32), out).astype(F32)


def dist2_of(points, q):
    """dot(p - q, p - q) in float32, as the query computes it."""
    with np.errstate(all="ignore"):
        d = np.asarray(points, F32).reshape(-1, 3) - q
        return D._dot(d, d).astype(F32)


# ------------------------------------------------------------------------------------------------ the shared meshes and points
def far_points(lo=D.LO, hi=D.HI):
    """Six points 100 box widths from the box, one beyond each side, and one beyond a corner."""
    lo, hi = np.array(lo, np.float64), np.array(hi, np.float64)
    ctr, ext = (lo + hi) / 2, hi - lo
    pts = []
    for a in range(3):
        for sgn in (-1.0, 1.0):
            p = ctr + 0.1 * ext * np.array([0.3, -0.2, 0.1])
            p[a] = (lo[a] if sgn < 0 else hi[a]) + sgn * 100.0 * ext[a]
            pts.append(p)
    pts.append(hi + 100.0 * ext)
    return np.array(pts, F32)


def small(F, seed=3):
    """A mesh of F small random triangles inside the box: the leaf and power-of-two edges."""
    rng = np.random.default_rng(seed + F)
    lo, hi = np.array(D.LO), np.array(D.HI)
    ctr = lo + (hi - lo) * rng.random((F, 3))
    v = (ctr[:, None, :] + 0.1 * rng.standard_normal((F, 3, 3))).reshape(-1, 3).astype(F32)
    return v, np.arange(3 * F, dtype=np.int32).reshape(-1, 3)


def all_invalid():
    """Five faces, none valid: bad indices, equal corners, a collinear one."""
    v = np.array([[0, 0, 1], [1, 0, 1], [2, 0, 1], [0, 1, 1]], F32)
    return v, np.array([[0, 1, 9], [0, 0, 1], [0, 1, 2], [-1, 1, 3], [3, 3, 3]], np.int32)


def doubled(name="sphere12"):
    """Every face listed twice, the copies behind the originals: the lower index must win every tie."""
    v, f = D.MESHES[name]()
    return v, np.concatenate([f, f]).astype(np.int32)
