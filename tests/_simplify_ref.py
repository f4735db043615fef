"""numpy reference of include/nerf_hip.h "mesh simplification" (a helper module, not a test): int64 accumulators, float64
placement in the header's operation order, operator for operator.  numpy evaluates every float64 operation separately (no fused
multiply-add), as the library does with -ffp-contract=off.  Also the small meshes the host and GPU tests share."""
import functools

import numpy as np

from tests import _mesh_ref as M

MEAN, QUADRIC = 0, 1
PLACEMENTS = {"mean": MEAN, "quadric": QUADRIC}
NO_KEY = np.iinfo(np.int64).max
_2_32, _2_30 = 4294967296.0, 1073741824.0


def _fix(x, lim, scale):
    """(int64)rint(min(max(x, -lim), lim) * scale), 0 for NaN."""
    x = np.asarray(x, np.float64)
    nan = np.isnan(x)
    y = np.minimum(np.maximum(np.where(nan, 0.0, x), -lim), lim)
    return np.where(nan, 0, np.rint(y * scale).astype(np.int64))


def cells(verts, G, lo, hi):
    """(t [V, 3] f64, q [V, 3] f64, valid [V], c [3], lo [3] f64)."""
    lo = np.asarray(lo, np.float32).astype(np.float64)
    hi = np.asarray(hi, np.float32).astype(np.float64)
    ext = hi - lo
    c = ext / float(G)
    inv = float(G) / ext
    with np.errstate(all="ignore"):
        t = (np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3) - lo) * inv
        valid = np.isfinite(t).all(1)
        q = np.minimum(np.maximum(np.floor(np.where(np.isnan(t), 0.0, t)), 0.0), float(G - 1))
    return t, q, valid, c, lo


def simplify(verts, faces, normals, colors, G, lo, hi, placement="quadric", info=None):
    """(verts' [V', 3] f32, faces' [F', 3] i32, normals' [V', 3] f32, colors' [V', 3] f32 or None).  `info` (a dict) receives
    K (clusters), keys (the int64 face keys) and keep (the survivor flags by input order)."""
    quadric = PLACEMENTS[placement] == QUADRIC
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    normals = np.asarray(normals, np.float32).reshape(-1, 3)
    V, F = len(verts), len(faces)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32),
             None if colors is None else np.zeros((0, 3), np.float32))
    if info is not None:
        info.update(K=0, keys=np.full(F, NO_KEY, np.int64), keep=np.zeros(F, bool))
    if V == 0 or F == 0:
        return empty
    t, q, valid, c, lo64 = cells(verts, G, lo, hi)
    qi = q.astype(np.int64)
    key = (qi[:, 2] * G + qi[:, 1]) * G + qi[:, 0]
    uk, inv_idx = np.unique(key[valid], return_inverse=True)
    K = len(uk)
    cid = np.full(V, -1, np.int64)
    cid[valid] = inv_idx
    vv = np.nonzero(valid)[0]
    # ---- vertex sums
    n = np.bincount(cid[vv], minlength=K).astype(np.int64)
    u = t[vv] - (q[vv] + 0.5)
    S = np.zeros((K, 3), np.int64)
    np.add.at(S, cid[vv], _fix(u, 64.0, _2_32))
    nrm = normals[vv].astype(np.float64)
    Ns = np.zeros((K, 3), np.int64)
    np.add.at(Ns, cid[vv], np.where(np.isfinite(nrm), _fix(np.where(np.isfinite(nrm), nrm, 0.0), 256.0, _2_30), 0))
    Cs = None
    if colors is not None:
        col = np.asarray(colors, np.float32).reshape(-1, 3)[vv].astype(np.float64)
        nan = np.isnan(col)
        ci = np.rint(np.minimum(np.maximum(np.where(nan, 0.0, col), 0.0), 1.0) * _2_30).astype(np.int64)
        Cs = np.zeros((K, 3), np.int64)
        np.add.at(Cs, cid[vv], np.where(nan, 0, ci))
    # ---- faces with three valid corners: quadrics once per distinct cluster
    f = faces.astype(np.int64)
    inr = ((f >= 0) & (f < V)).all(1)
    fs = np.where(inr[:, None], f, 0)
    ok = inr & (cid[fs] >= 0).all(1)
    fo = f[ok]
    g = cid[fo]
    Q = np.zeros((K, 9), np.int64)
    with np.errstate(all="ignore"):
        for corner in range(3):
            first = np.ones(len(fo), bool)
            for prev in range(corner):
                first &= g[:, prev] != g[:, corner]
            qc = q[fo[:, corner]]
            u0, u1, u2 = (t[fo[:, j]] - (qc + 0.5) for j in range(3))
            e1, e2 = u1 - u0, u2 - u0
            nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            d = -((nx * u0[:, 0] + ny * u0[:, 1]) + nz * u0[:, 2])
            x = np.stack([nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, nx * d, ny * d, nz * d], 1)
            np.add.at(Q, g[first, corner], _fix(x, 64.0, _2_32)[first])
    # ---- placement
    nf = n.astype(np.float64)
    ub = S.astype(np.float64) / _2_32 / nf[:, None]
    x = ub.copy()
    if quadric:
        with np.errstate(all="ignore"):
            A = Q.astype(np.float64) / _2_32
            tr = (A[:, 0] + A[:, 3]) + A[:, 5]
            mu = (tr / 3.0) * 0.0009765625
            a00, a01, a02, a11, a12, a22 = A[:, 0] + mu, A[:, 1], A[:, 2], A[:, 3] + mu, A[:, 4], A[:, 5] + mu
            r0, r1, r2 = mu * ub[:, 0] - A[:, 6], mu * ub[:, 1] - A[:, 7], mu * ub[:, 2] - A[:, 8]
            c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
            c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
            det = (a00 * c00 + a01 * c01) + a02 * c02
            s = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                          ((c02 * r0 + c12 * r1) + c22 * r2) / det], 1)
            take = (tr > 0.0) & np.isfinite(s).all(1) & (np.abs(s) <= 0.5).all(1)
        x[take] = s[take]
    qk = np.stack([uk % G, (uk // G) % G, uk // (G * G)], 1).astype(np.float64)
    nv = (lo64 + ((qk + 0.5) + x) * c).astype(np.float32)
    sN = Ns.astype(np.float64) / _2_30
    ln = np.sqrt((sN[:, 0] * sN[:, 0] + sN[:, 1] * sN[:, 1]) + sN[:, 2] * sN[:, 2])
    with np.errstate(all="ignore"):
        nn = np.where(ln[:, None] > 0.0, sN / ln[:, None], 0.0).astype(np.float32)
    nc = None if Cs is None else (Cs.astype(np.float64) / _2_30 / nf[:, None]).astype(np.float32)
    # ---- faces: keys, runs, survivors
    keys = np.full(F, NO_KEY, np.int64)
    odd = np.zeros(F, np.int64)
    nd = (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    srt = np.sort(g, 1)
    okidx = np.nonzero(ok)[0]
    keys[okidx[nd]] = ((srt[nd, 0] << 42) | (srt[nd, 1] << 21) | srt[nd, 2])
    odd[okidx] = ((g[:, 0] < g[:, 1]).astype(np.int64) + (g[:, 1] < g[:, 2]) + (g[:, 0] < g[:, 2])) & 1
    perm = np.argsort(keys, kind="stable")
    sk = keys[perm]
    so = np.where(sk != NO_KEY, odd[perm], 0)
    head = np.ones(F, bool)
    head[1:] = sk[1:] != sk[:-1]
    rid = np.cumsum(head) - 1
    heads = np.append(np.nonzero(head)[0], F)
    pre = np.append(0, np.cumsum(so))                               # odd faces below a position
    s_, e_ = heads[rid], heads[rid + 1]
    m = pre[e_] - pre[s_]
    p = (e_ - s_) - m
    below = pre[np.arange(F)] - pre[s_]
    rank = np.where(so == 1, below, (np.arange(F) - s_) - below)
    keep = np.zeros(F, bool)
    keep[perm] = (sk != NO_KEY) & (rank >= np.minimum(p, m))
    if info is not None:
        info.update(K=K, keys=keys, keep=keep)
    # ---- compaction
    gf = np.full((F, 3), -1, np.int64)
    gf[okidx] = g
    g2 = gf[keep]
    used = np.zeros(K, bool)
    used[g2.ravel()] = True
    new = np.cumsum(used) - 1
    return nv[used], new[g2].astype(np.int32).reshape(-1, 3), nn[used], None if nc is None else nc[used]


# ------------------------------------------------------------------------------------------------ the shared meshes
LO, HI = [-1.0] * 3, [1.0] * 3
GRIDS = (4, 8, 12)
BOX_C, BOX_H = np.array([0.03, 0.02, -0.04]), np.array([0.55, 0.4, 0.3])


def _vol(R, fn):
    p = M.lattice_points(R, LO, HI).astype(np.float64)
    return fn(p).reshape(R, R, R).astype(np.float32)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(verts, faces, normals, colors) of one of: sphere, box, plate (R = 32), noise (R = 16, iso 0.3, open at the border),
    small (a sphere of radius 0.2 inside one cell of G = 2).  Colours: a fixed function of the position with values outside [0, 1]."""
    if name == "noise":
        vol, iso = np.random.default_rng(1).standard_normal((16, 16, 16)).astype(np.float32), 0.3
    else:
        fn = {"sphere": lambda p: 0.6 - np.linalg.norm(p - [0.1, -0.05, 0.05], axis=1),
              "small": lambda p: 0.2 - np.linalg.norm(p - [0.5, 0.5, 0.5], axis=1),
              "box": lambda p: -np.max(np.abs(p - BOX_C) - BOX_H, axis=1),
              "plate": lambda p: ((np.abs(p[:, 2] - 0.28) < 0.04) & (np.abs(p[:, 0]) < 0.6) & (np.abs(p[:, 1]) < 0.6)).astype(float)}
        vol, iso = _vol(32, fn[name]), 0.5 if name == "plate" else 0.0
    v, f, n = M.marching_cubes(vol, iso, LO, HI)
    col = (0.5 + 0.7 * np.sin(3.0 * v.astype(np.float64) + [0.0, 1.0, 2.0])).astype(np.float32)
    for a in (v, f, n, col):
        a.setflags(write=False)
    return v, f, n, col


@functools.lru_cache(maxsize=None)
def expected(name, G, placement, with_colors):
    v, f, n, col = mesh(name)
    info = {}
    out = simplify(v, f, n, col if with_colors else None, G, LO, HI, placement, info)
    return out, info


def box_errors(verts):
    """(worst distance from a true corner of the box to the nearest vertex, worst |signed distance| of a vertex to the box)."""
    v = np.asarray(verts, np.float64)
    corners = np.array([BOX_C + np.array(s) * BOX_H for s in [(i, j, k) for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)]])
    dc = max(float(np.linalg.norm(v - cc, axis=1).min()) for cc in corners)
    qd = np.abs(v - BOX_C) - BOX_H
    sd = np.linalg.norm(np.maximum(qd, 0.0), axis=1) + np.minimum(qd.max(1), 0.0)
    return dc, float(np.abs(sd).max())
