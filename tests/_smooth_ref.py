"""numpy reference of include/nerf_hip.h "mesh smoothing" (a helper module, not a test): rows built with np.add.at, int64 sums,
float64 arithmetic in the header's operation order, operator for operator.  numpy evaluates every float64 operation separately (no
fused multiply-add), as the library does with -ffp-contract=off.  Also the small meshes the host and GPU tests share."""
import functools

import numpy as np

from tests import _mesh_ref as M

POS_LIM, POS_SCALE = 4.0, 4294967296.0              # fix(u, 4, 2^32)
NRM_LIM, NRM_SCALE = 16.0, 17179869184.0            # fix(c, 16, 2^34)
MAX_ITERATIONS = 1024
LAM, MU = 0.5, -0.53


def _fix(x, lim, scale):
    """(int64)rint(min(max(x, -lim), lim) * scale), 0 for NaN."""
    x = np.asarray(x, np.float64)
    nan = np.isnan(x)
    y = np.minimum(np.maximum(np.where(nan, 0.0, x), -lim), lim)
    return np.where(nan, 0, np.rint(y * scale).astype(np.int64))


def box(lo, hi):
    """(ctr [3], ext [3]) float64 of the float32 box."""
    lo = np.asarray(lo, np.float32).astype(np.float64)
    hi = np.asarray(hi, np.float32).astype(np.float64)
    return (lo + hi) * 0.5, hi - lo


def entries(faces, V):
    """(row [E], b [E], c [E]) int64: the entries of the faces that are not ignored, row a receiving (b, c), row b (c, a), row c
    (a, b)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    f = f[ok]
    return (np.concatenate([f[:, 0], f[:, 1], f[:, 2]]), np.concatenate([f[:, 1], f[:, 2], f[:, 0]]),
            np.concatenate([f[:, 2], f[:, 0], f[:, 1]]))


def half_step(verts, ent, ctr, ext, k):
    """One half-step with the float32 factor k on float32 positions [V, 3]."""
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    V = len(v32)
    row, b, c = ent
    fin = np.isfinite(v32).all(1)
    v = v32.astype(np.float64)
    S = np.zeros((V, 3), np.int64)
    n = np.zeros(V, np.int64)
    with np.errstate(all="ignore"):
        for nb in (b, c):
            take = fin[nb]
            u = (v[nb[take]] - ctr) / ext
            np.add.at(S, row[take], _fix(u, POS_LIM, POS_SCALE))
            np.add.at(n, row[take], 1)
        move = fin & (n > 0)
        nn = np.where(move, n, 1).astype(np.float64)
        mean = ctr + (S.astype(np.float64) / POS_SCALE / nn[:, None]) * ext
        kk = float(np.float32(k))
        new = (v + kk * (mean - v)).astype(np.float32)
    out = v32.copy()
    out[move] = new[move]
    return out


def normals(verts, ent, ctr, ext):
    """float32 [V, 3]: the normalised area-weighted sums of the face normals around each vertex, 0 where there is none."""
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    V = len(v32)
    row, b, c = ent
    fin = np.isfinite(v32).all(1)
    v = v32.astype(np.float64)
    take = fin[row] & fin[b] & fin[c]
    r, b, c = row[take], b[take], c[take]
    N = np.zeros((V, 3), np.int64)
    with np.errstate(all="ignore"):
        d1 = (v[b] - v[r]) / ext
        d2 = (v[c] - v[r]) / ext
        cr = np.stack([d1[:, 1] * d2[:, 2] - d1[:, 2] * d2[:, 1], d1[:, 2] * d2[:, 0] - d1[:, 0] * d2[:, 2],
                       d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]], 1)
        np.add.at(N, r, _fix(cr, NRM_LIM, NRM_SCALE))
        w = np.array([ext[1] * ext[2], ext[2] * ext[0], ext[0] * ext[1]])
        s = (N.astype(np.float64) / NRM_SCALE) * w
        ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        return np.where(ln[:, None] > 0.0, s / ln[:, None], 0.0).astype(np.float32)


def color_rows(verts, nrm):
    """float32 [V, 11]: [x, -n, 0, 0, -n]."""
    rows = np.zeros((len(verts), 11), np.float32)
    rows[:, 0:3] = verts
    rows[:, 3:6] = -nrm
    rows[:, 8:11] = -nrm
    return rows


def smooth(verts, faces, iterations, lo, hi, lam=LAM, mu=MU):
    """(verts' [V, 3] f32, normals' [V, 3] f32) after `iterations` pairs (mu = 0: single lambda half-steps)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).copy()
    ent = entries(faces, len(v))
    ctr, ext = box(lo, hi)
    for _ in range(int(iterations)):
        v = half_step(v, ent, ctr, ext, lam)
        if float(np.float32(mu)) != 0.0:
            v = half_step(v, ent, ctr, ext, mu)
    return v, normals(v, ent, ctr, ext)


def roughness(verts, faces):
    """The mean distance of a (referenced) vertex from the face-weighted mean of its neighbours, float64."""
    v = np.asarray(verts, np.float64)
    row, b, c = entries(faces, len(v))
    S = np.zeros((len(v), 3))
    n = np.zeros(len(v))
    for nb in (b, c):
        np.add.at(S, row, v[nb])
        np.add.at(n, row, 1.0)
    use = n > 0
    return float(np.linalg.norm(S[use] / n[use, None] - v[use], axis=1).mean())


# ------------------------------------------------------------------------------------------------ the shared meshes
LO, HI = [-1.5, -0.7, 0.1], [1.5, 2.3, 3.1]
CENTRE, RADIUS, NOISE = np.array([0.0, 0.8, 1.6]), 1.0, 0.08


@functools.lru_cache(maxsize=None)
def sphere(R):
    """(verts, faces) of marching cubes at iso 0 of RADIUS - |p - CENTRE| + NOISE * standard_normal (default_rng(R)) on the R^3
    lattice of the box: closed, rough at the scale of a cell."""
    p = M.lattice_points(R, LO, HI).astype(np.float64)
    noise = np.random.default_rng(R).standard_normal(R ** 3)
    vol = (RADIUS - np.linalg.norm(p - CENTRE, axis=1) + NOISE * noise).reshape(R, R, R).astype(np.float32)
    v, f, _ = M.marching_cubes(vol, 0.0, LO, HI)
    for a in (v, f):
        a.setflags(write=False)
    return v, f


def tetrahedron():
    v = np.array([[0.0, 0.8, 2.4], [0.9, 0.8, 1.2], [-0.5, 1.6, 1.2], [-0.5, 0.0, 1.3]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]], np.int32)
    return v, f


def strip(n=40):
    """An open zig-zag strip of n triangles with seeded bumps: boundary edges everywhere (weight 1), interior ones between."""
    rng = np.random.default_rng(3)
    k = np.arange(n + 2)
    v = np.stack([-1.2 + 2.4 * k / (n + 1), 0.8 + 0.3 * (k % 2), 1.6 + 0.05 * rng.standard_normal(n + 2)], 1).astype(np.float32)
    f = np.array([[i, i + 1, i + 2] if i % 2 == 0 else [i + 1, i, i + 2] for i in range(n)], np.int32)
    return v, f


def fan(valence=300):
    """A closed fan: a hub of the given valence over a bumpy rim.  The hub's row is longer than a wave and than a workgroup."""
    rng = np.random.default_rng(4)
    t = 2.0 * np.pi * np.arange(valence) / valence
    rim = np.stack([np.cos(t), 0.8 + np.sin(t), 1.6 + 0.1 * rng.standard_normal(valence)], 1)
    v = np.concatenate([[[0.02, 0.83, 2.0]], rim]).astype(np.float32)
    i = np.arange(valence)
    f = np.stack([np.zeros(valence, np.int64), 1 + i, 1 + (i + 1) % valence], 1).astype(np.int32)
    return v, f


def grid_mesh(nx, ny, bump=0.05, seed=5, flat=False):
    """An nx x ny vertex sheet, two triangles per quad in alternating diagonals, seeded bumps along z unless `flat`."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    z = np.zeros(nx * ny) if flat else bump * rng.standard_normal(nx * ny)
    v = np.stack([-1.0 + 2.0 * i.ravel() / (nx - 1), 0.0 + 2.0 * j.ravel() / (ny - 1), 1.5 + z], 1).astype(np.float32)
    idx = lambda a, b: a * ny + b
    f = []
    for a in range(nx - 1):
        for b in range(ny - 1):
            p, q, r, s = idx(a, b), idx(a + 1, b), idx(a + 1, b + 1), idx(a, b + 1)
            f += [[p, q, r], [p, r, s]] if (a + b) % 2 == 0 else [[p, q, s], [q, r, s]]
    return v, np.array(f, np.int32)


def junk(R=12):
    """The noisy sphere with appended ignored faces (indices out of range, equal corners), one vertex with a NaN coordinate
    and one unreferenced vertex at the end.  -> (verts, faces, index of the NaN vertex, index of the unreferenced vertex)."""
    v, f = sphere(R)
    V = len(v)
    v = np.concatenate([v, [[0.3, 0.9, 1.7]]]).astype(np.float32)
    bad = np.array([[0, 1, V + 1], [-1, 2, 3], [4, 4, 5], [6, 7, 6], [8, 9, 9], [np.iinfo(np.int32).max, 0, 1],
                    [np.iinfo(np.int32).min, 3, 2], [V + 5, V + 5, V + 5]], np.int32)
    f = np.concatenate([f[:100], bad[:4], f[100:], bad[4:]]).astype(np.int32)
    v[17, 1] = np.nan
    return v, f, 17, V
