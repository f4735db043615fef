"""numpy reference of include/nerf_hip.h "mesh winding number" (a helper module, not a test): the moments of every node of the face
hierarchy from tests/_bvh_ref.py's nodes and order, the walk that replaces far subtrees by their dipole -- emulated point by point,
with its two counters -- and the exact sum in face order.  Everything is IEEE float64 on the float32 corners and points with one
operation per operator: the moments and the face-order sum as float64 numpy arrays, the walk on Python floats (the same IEEE
doubles; math.sqrt is correctly rounded), because it runs node by node.  The only operation a device may round differently is
atan2, once per exact term."""
import math

import numpy as np

from tests import _bvh_ref as B
from tests import _distance_ref as D
from tests import _mesh_ref as M

F32, F64 = np.float32, np.float64
NODE_DOUBLES = 12
N_AT, C_AT, R_AT, A_AT, S_AT = 0, 3, 6, 7, 8
FOUR_PI = 4.0 * math.pi                                 # exact: a power of two times the double pi


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def face_terms(a, b, c):
    """(n_f [F, 3], a_f [F], a_f ((a + b) + c) / 3 [F, 3]) in float64 from float32 corners."""
    a, b, c = (np.asarray(x, F32).astype(F64) for x in (a, b, c))
    n = 0.5 * _cross(b - a, c - a)
    af = np.sqrt(_dot(n, n))
    return n, af, (af[:, None] * ((a + b) + c)) / 3.0


def _records(N, S, A, box):
    """[k, 12] records from the sums and the float32 boxes [k, 6]; zeros for an empty node."""
    mn, mx = box[:, :3].astype(F64), box[:, 3:].astype(F64)
    empty = box[:, 0] > box[:, 3]
    with np.errstate(all="ignore"):
        c = np.where((A == 0.0)[:, None], (mn + mx) * 0.5, S / A[:, None])
        e = np.fmax(c - mn, mx - c)
        r = np.sqrt(_dot(e, e))
    out = np.zeros((len(A), NODE_DOUBLES), F64)
    out[:, N_AT:N_AT + 3], out[:, C_AT:C_AT + 3], out[:, R_AT], out[:, A_AT], out[:, S_AT:S_AT + 3] = N, c, r, A, S
    out[empty] = 0.0
    return out


def moments(tree):
    """float64 [2 P, 12] per node in heap order: N [0:3], c [3:6], r [6], A [7], S [8:11], 0.  A leaf adds its valid faces in
    sorted order; an internal node is left + right; node 0 is zeros."""
    P, F = tree.P, tree.F
    n, af, sc = face_terms(tree.a, tree.b, tree.c)
    out = np.zeros((2 * P, NODE_DOUBLES), F64)
    N, S, A = np.zeros((P, 3), F64), np.zeros((P, 3), F64), np.zeros(P, F64)
    slots = np.concatenate([tree.order, np.full(B.LEAF * P - F, -1, np.int32)]).reshape(P, B.LEAF)
    for k in range(B.LEAF if F else 0):
        ok = slots[:, k] >= 0
        g = np.where(ok, slots[:, k], 0)
        N = np.where(ok[:, None], N + n[g], N)
        S = np.where(ok[:, None], S + sc[g], S)
        A = np.where(ok, A + af[g], A)
    out[P:] = _records(N, S, A, tree.nodes[P:])
    first = P // 2
    while first >= 1:
        i = np.arange(first, 2 * first)
        l, r = out[2 * i], out[2 * i + 1]
        out[i] = _records(l[:, N_AT:N_AT + 3] + r[:, N_AT:N_AT + 3], l[:, S_AT:S_AT + 3] + r[:, S_AT:S_AT + 3],
                          l[:, A_AT] + r[:, A_AT], tree.nodes[i])
        first //= 2
    return out


def solid_angle(q, a, b, c):
    """2 atan2(det, den) of one triangle seen from q, on Python floats; 0 where det == 0 (q in the plane of the face)."""
    x0, x1, x2 = a[0] - q[0], a[1] - q[1], a[2] - q[2]
    y0, y1, y2 = b[0] - q[0], b[1] - q[1], b[2] - q[2]
    z0, z1, z2 = c[0] - q[0], c[1] - q[1], c[2] - q[2]
    lx = math.sqrt((x0 * x0 + x1 * x1) + x2 * x2)
    ly = math.sqrt((y0 * y0 + y1 * y1) + y2 * y2)
    lz = math.sqrt((z0 * z0 + z1 * z1) + z2 * z2)
    c0, c1, c2 = y1 * z2 - y2 * z1, y2 * z0 - y0 * z2, y0 * z1 - y1 * z0
    det = (x0 * c0 + x1 * c1) + x2 * c2
    if det == 0.0:
        return 0.0
    xy = (x0 * y0 + x1 * y1) + x2 * y2
    yz = (y0 * z0 + y1 * z1) + y2 * z2
    zx = (z0 * x0 + z1 * x1) + z2 * x2
    den = (((lx * ly) * lz + xy * lz) + yz * lx) + zx * ly
    return 2.0 * math.atan2(det, den)


def exact_sum(points, verts, faces):
    """float64 [n]: the sum of the solid angles of the valid faces in face order, over 4 pi; NaN for a non-finite point.  numpy,
    one face per column, added left to right."""
    pts = np.asarray(points, F32).reshape(-1, 3)
    ok, a, b, c, _ = D.corners(verts, faces)
    a, b, c = (x[ok].astype(F64) for x in (a, b, c))
    fin = np.isfinite(pts).all(1)
    q = np.where(fin[:, None], pts, F32(0)).astype(F64)[:, None, :]
    w = np.zeros(len(pts), F64)
    if len(a) and len(pts):
        with np.errstate(all="ignore"):
            x, y, z = a[None] - q, b[None] - q, c[None] - q
            lx, ly, lz = np.sqrt(_dot(x, x)), np.sqrt(_dot(y, y)), np.sqrt(_dot(z, z))
            det = _dot(x, _cross(y, z))
            den = (((lx * ly) * lz + _dot(x, y) * lz) + _dot(y, z) * lx) + _dot(z, x) * ly
            om = np.where(det == 0.0, 0.0, 2.0 * np.arctan2(det, den))
        w = np.cumsum(om, axis=1)[:, -1] / FOUR_PI
    return np.where(fin, w, np.nan)


class Winding:
    """The moments of one mesh on its hierarchy, built once; query() walks it for every point."""

    def __init__(self, verts, faces, lo=D.LO, hi=D.HI, tree=None):
        self.tree = tree if tree is not None else B.Tree(verts, faces, lo, hi)
        t = self.tree
        self.P, self.F = t.P, t.F
        self.moments = moments(t)
        self.valid = int((t.order >= 0).sum())
        # plain Python values for the scalar walk
        self._mom = self.moments[:, :R_AT + 1].tolist()
        self._empty = (t.nodes[:, 0] > t.nodes[:, 3]).tolist()
        self._order = t.order.tolist()
        self._a, self._b, self._c = (x.astype(F64).tolist() for x in (t.a, t.b, t.c))

    def one(self, p, beta):
        """(w, faces evaluated exactly, nodes approximated) for one finite float32 point: the kernel's walk, step for step."""
        q = [float(x) for x in np.asarray(p, F32)]
        b2 = float(beta) * float(beta)
        s, exact, approx = 0.0, 0, 0
        node, P, F = 1, self.P, self.F
        while True:
            down = False
            if self._empty[node]:
                pass
            elif node >= P:
                s0 = B.LEAF * (node - P)
                for slot in range(s0, min(s0 + B.LEAF, F)):
                    f = self._order[slot]
                    if f < 0:
                        continue
                    s += solid_angle(q, self._a[f], self._b[f], self._c[f])
                    exact += 1
            else:
                m = self._mom[node]
                d0, d1, d2 = m[C_AT] - q[0], m[C_AT + 1] - q[1], m[C_AT + 2] - q[2]
                dd = (d0 * d0 + d1 * d1) + d2 * d2
                r = m[R_AT]
                if dd > b2 * (r * r):                                  # strict; a NaN product (inf 0) never approximates
                    s += ((m[N_AT] * d0 + m[N_AT + 1] * d1) + m[N_AT + 2] * d2) / (dd * math.sqrt(dd))
                    approx += 1
                else:
                    down = True
            if down:
                node *= 2
                continue
            while node & 1:
                node >>= 1
            if node == 0:
                break
            node += 1
        return s / FOUR_PI, exact, approx

    def query(self, points, beta=2.0):
        """(w [n] float64, visits [n, 2] int32): (NaN, 0, 0) for a non-finite point."""
        pts = np.asarray(points, F32).reshape(-1, 3)
        w, visits = np.full(len(pts), np.nan, F64), np.zeros((len(pts), 2), np.int32)
        for i in np.nonzero(np.isfinite(pts).all(1))[0]:
            w[i], visits[i, 0], visits[i, 1] = self.one(pts[i], beta)
        return w, visits

    def volume(self, R, lo, hi, beta=2.0):
        """float32 [R, R, R]: w on the lattice of the box, rounded once; also the float64 values."""
        w, _ = self.query(M.lattice_points(R, lo, hi), beta)
        return w.astype(F32).reshape(R, R, R), w.reshape(R, R, R)


# ------------------------------------------------------------------------------------------------ the shared meshes
def open_cube():
    """D.cube() without its last two faces: a square hole with 4 boundary edges."""
    v, f = D.cube()
    return v, f[:-2].copy()


def octant_triangle(flip=False):
    """One triangle with its corners at unit distance on the three axes: it covers an eighth of the sphere seen from the origin."""
    v = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], F32)
    return v, np.array([[0, 2, 1] if flip else [0, 1, 2]], np.int32)
