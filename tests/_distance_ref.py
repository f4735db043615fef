"""numpy reference of include/nerf_hip.h "mesh distance" (a helper module, not a test): the validity and weight rule, the int64 CDF,
the counter-based draws and the sampled point; Ericson's point-triangle routine in float32, operator for operator; and the brute
force over every face with the lowest-index tie rule.  numpy evaluates every float32 operation separately (no fused multiply-add),
as the library does with -ffp-contract=off; divisions and the root go through float64 and are rounded once.  Also the small meshes
and point sets the host and GPU tests share."""
import numpy as np

from tests import _smooth_ref as S

F32 = np.float32
W_LIM, W_SCALE = 16.0, 17179869184.0                # weight = max(1, rint(min(d / U, 16) 2^34))
MAX_GRID = 256
GOLD, SALT = 0x9E3779B97F4A7C15, 0x632BE59BD9B4E019
MASK = (1 << 64) - 1
NAN_BITS = 0x7FC00000


def _div(a, b):
    """a / b correctly rounded to float32."""
    with np.errstate(all="ignore"):
        return (a.astype(np.float64) / b.astype(np.float64)).astype(F32)


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def corners(verts, faces):
    """(valid [F] bool, a, b, c [F, 3] float32, doubled area [F] float32); the corners of an invalid face are zeros."""
    v = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    ok = ((f >= 0) & (f < V)).all(1)
    g = np.where(ok[:, None], f, 0)
    if V == 0:
        z = np.zeros((len(f), 3), F32)
        return np.zeros(len(f), bool), z, z, z, np.zeros(len(f), F32)
    a, b, c = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    ok &= np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1)
    a, b, c = (np.where(ok[:, None], x, F32(0)) for x in (a, b, c))
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        ok &= (n != 0).any(1)
        d = np.sqrt(((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).astype(np.float64)).astype(F32)
    return ok, a, b, c, d


def weights(verts, faces, lo, hi):
    """int64 [F]: 0 for an invalid face, else max(1, rint(min(d / U, 16) 2^34)), U the largest extent squared."""
    ok, _, _, _, d = corners(verts, faces)
    ext = np.asarray(hi, F32).astype(np.float64) - np.asarray(lo, F32).astype(np.float64)
    U = ext.max() * ext.max()
    with np.errstate(all="ignore"):
        x = d.astype(np.float64) / U
    x = np.where(x < W_LIM, x, W_LIM)
    w = np.maximum(np.rint(x * W_SCALE).astype(np.int64), 1)
    return np.where(ok, w, 0)


def cdf(verts, faces, lo, hi):
    return np.cumsum(weights(verts, faces, lo, hi), dtype=np.int64)


def mix64(z):
    """The splitmix64 finaliser on Python ints."""
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draws(seed, i):
    key = mix64(seed ^ mix64(i + SALT))
    return tuple(mix64(key + (j + 1) * GOLD) for j in range(3))


def sample(verts, faces, n, lo, hi, seed=0):
    """(points [n, 3] float32, face [n] int32, u [n, 2] float32) of samples 0 .. n - 1."""
    _, a, b, c, _ = corners(verts, faces)
    cd = cdf(verts, faces, lo, hi)
    total = int(cd[-1]) if len(cd) else 0
    if n and total <= 0:
        raise ValueError("the mesh has no area")
    face = np.zeros(n, np.int32)
    u = np.zeros((n, 2), F32)
    for i in range(n):
        r0, r1, r2 = draws(seed, i)
        target = (r0 * total) >> 64
        face[i] = int(np.searchsorted(cd, target, side="right"))     # the first f with cdf_f > target
        A, B = r1 >> 40, r2 >> 40
        if A + B > 1 << 24:
            A, B = (1 << 24) - A, (1 << 24) - B
        u[i] = F32(A) * F32(2.0 ** -24), F32(B) * F32(2.0 ** -24)
    fa, fb, fc = a[face], b[face], c[face]
    pts = (fa + u[:, :1] * (fb - fa)) + u[:, 1:] * (fc - fa)
    return pts.astype(F32), face, u


def point_triangle_d2(p, a, b, c):
    """float32 squared distance from p [..., 3] to the triangles (a, b, c) [..., 3] (broadcast), the header's rule."""
    p, a, b, c = (np.asarray(x, F32) for x in (p, a, b, c))
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp, bc = b - a, c - a, p - a, p - b, p - c, c - b
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        s = (va + vb) + vc
        v_in, w_in = _div(vb, s), _div(vc, s)
        q = (a + v_in[..., None] * ab) + w_in[..., None] * ac                                           # interior
        tests = [(va <= 0) & (e43 >= 0) & (e56 >= 0), (vb <= 0) & (d2 >= 0) & (d6 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d3 >= 0) & (d4 <= d3), (d1 <= 0) & (d2 <= 0)]
        points = [b + _div(e43, e43 + e56)[..., None] * bc, a + _div(d2, d2 - d6)[..., None] * ac, np.broadcast_to(c, q.shape),
                  a + _div(d1, d1 - d3)[..., None] * ab, np.broadcast_to(b, q.shape), np.broadcast_to(a, q.shape)]
        for t, x in zip(tests, points):                                # the last assignment wins: the header's first test
            q = np.where(t[..., None], x, q)
        d = p - q
        return _dot(d, d).astype(F32)


def brute_force(points, verts, faces, chunk=512):
    """(dist2 [n] float32, face [n] int32): the minimum over every valid face of the key (bits of D) 2^32 + f."""
    pts = np.asarray(points, F32).reshape(-1, 3)
    ok, a, b, c, _ = corners(verts, faces)
    idx = np.nonzero(ok)[0].astype(np.uint64)
    a, b, c = a[ok], b[ok], c[ok]
    n = len(pts)
    none = np.uint64((0x7F800000 << 32) | 0xFFFFFFFF)
    best = np.full(n, none, np.uint64)
    fin = np.isfinite(pts).all(1)
    if len(idx):
        for s in range(0, n, chunk):
            d = point_triangle_d2(pts[s:s + chunk, None, :], a[None], b[None], c[None])
            key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx[None]
            key = np.where(np.isnan(d), none, key)
            best[s:s + chunk] = np.minimum(key.min(1), none)
    bits = (best >> np.uint64(32)).astype(np.uint32)
    face = (best & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32).copy()
    bits[~fin] = NAN_BITS
    face[~fin] = -1
    return bits.view(F32), face


def default_grid(F):
    """The grid MeshIndex picks: isqrt(F // 32) clamped to [1, 256]."""
    return int(min(MAX_GRID, max(1, int(np.floor(np.sqrt(F // 32))))))


# ------------------------------------------------------------------------------------------------ the shared meshes and points
LO, HI = S.LO, S.HI


def cube(shift=0.0):
    """The 12-face cube [-0.5, 0.5]^3 + (shift, 0.75, 1.5): every coordinate a small binary fraction."""
    c = np.array([[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)], np.float64)
    v = (c + [shift, 0.75, 1.5]).astype(F32)
    f = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                  [1, 3, 5], [3, 7, 5]], np.int32)
    return v, f


def junk():
    """S.junk(12) (faces with bad indices and equal corners, a NaN vertex) plus two faces that are degenerate without equal
    indices: three collinear vertices, and two distinct vertices at the same place."""
    v, f, _, _ = S.junk(12)
    V = len(v)
    v = np.concatenate([v, [[0.0, 0.5, 1.0], [0.25, 0.5, 1.0], [0.5, 0.5, 1.0], [0.25, 0.5, 1.0]]]).astype(F32)
    f = np.concatenate([f[:7], [[V, V + 1, V + 2]], f[7:], [[V, V + 1, V + 3]]]).astype(np.int32)
    return v, f


def spanning():
    """One face across the whole box (first in the list) and 200 tiny ones: the entries exceed F and every cell has one."""
    rng = np.random.default_rng(21)
    lo, hi = np.array(LO), np.array(HI)
    big = np.array([[lo[0], lo[1], lo[2]], [hi[0], hi[1], lo[2]], [lo[0], hi[1], hi[2]]])
    ctr = lo + (hi - lo) * rng.random((200, 3))
    tiny = ctr[:, None, :] + 0.01 * rng.standard_normal((200, 3, 3))
    v = np.concatenate([big, tiny.reshape(-1, 3)]).astype(F32)
    f = np.arange(3 * 201, dtype=np.int32).reshape(-1, 3)
    return v, f


def outside():
    """A tetrahedron inside the box, one face wholly outside it and one that straddles its boundary."""
    v, f = S.tetrahedron()
    V = len(v)
    extra = np.array([[4.0, 5.0, 6.0], [5.0, 5.0, 6.5], [4.0, 6.0, 7.0], [1.0, 1.0, 2.0], [2.5, 1.0, 2.0], [1.0, 3.5, 4.0]], F32)
    return np.concatenate([v, extra]).astype(F32), np.concatenate([f, [[V, V + 1, V + 2], [V + 3, V + 4, V + 5]]]).astype(np.int32)


MESHES = {"tetrahedron": S.tetrahedron, "sphere12": lambda: S.sphere(12), "sphere24": lambda: S.sphere(24), "junk": junk,
          "spanning": spanning, "outside": outside}


def query_points(verts, faces, n, seed):
    """n float32 points: every (finite) mesh vertex and the midpoints of face edges first, then points outside the box on each of
    its six sides, one NaN point, and seeded points in a box half as large again; cut or padded to n."""
    v = np.asarray(verts, F32)
    ok, a, b, c, _ = corners(verts, faces)
    lo, hi = np.array(LO), np.array(HI)
    rng = np.random.default_rng(seed)
    mid = ((a[ok] + b[ok]) * F32(0.5))[:40]
    out = np.array([[lo[0] - 0.7, 0.8, 1.6], [hi[0] + 0.4, 0.9, 1.5], [0.1, lo[1] - 1.3, 1.7], [0.0, hi[1] + 0.2, 1.4],
                    [0.2, 0.7, lo[2] - 0.6], [-0.1, 0.8, hi[2] + 2.5], [hi[0] + 1.0, hi[1] + 1.0, hi[2] + 1.0]])
    nan = np.array([[0.1, np.nan, 1.0]])
    special = np.concatenate([out, nan, v[np.isfinite(v).all(1)][:120], mid])
    ctr, half = (lo + hi) / 2, (hi - lo) / 2
    rnd = ctr + 1.5 * half * (2.0 * rng.random((max(n, 1), 3)) - 1.0)
    pts = np.concatenate([special, rnd])[:n] if n > 8 else np.concatenate([rnd[:max(n - 1, 0)], v[:1]])[:n]
    return np.ascontiguousarray(pts, F32)
