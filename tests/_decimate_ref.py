"""numpy reference of include/nerf_hip.h "edge-collapse decimation" (a helper module, not a test): the same rounds, float64
arithmetic in the header's operation order, operator for operator, one rounding per operation.  numpy evaluates every float64
operation separately (no fused multiply-add), as the library does with -ffp-contract=off.  Every round is vectorised over the
edges and over the (edge, incident face) pairs: none of its checks depends on the order inside a ring.  Also the meshes the host
and GPU tests share."""
import functools

import numpy as np

from tests import _simplify_ref as S
from tests import _smooth_ref as SM

PLACEMENTS = {"midpoint": 0, "quadric": 1}            # NERF_DECIMATE_MIDPOINT / NERF_DECIMATE_QUADRIC
STOPS = ("target", "selected nothing", "max_rounds")  # the stop codes 0, 1, 2
MULT = 0x9E3779B1
NOKEY = np.uint64(2 ** 63 - 1)
LO, HI = S.LO, S.HI
M24 = (1 << 24) - 1


def box(lo, hi):
    """(ctr [3], hs) float64 of the float32 box: the centre and half the longest side."""
    lo = np.asarray(lo, np.float32).astype(np.float64)
    hi = np.asarray(hi, np.float32).astype(np.float64)
    return (lo + hi) * 0.5, np.max(hi - lo) * 0.5


def _cross(e1, e2):
    return (e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
            e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])


def face_quadrics(u, fin, faces):
    """[F, 10] (A 6, b 3, c 1): the area^2-weighted plane quadric of every face whose three corners are finite, 0 for the others."""
    u0, u1, u2 = u[faces[:, 0]], u[faces[:, 1]], u[faces[:, 2]]
    nx, ny, nz = _cross(u1 - u0, u2 - u0)
    d = -((nx * u0[:, 0] + ny * u0[:, 1]) + nz * u0[:, 2])
    K = np.stack([nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, nx * d, ny * d, nz * d, d * d], 1)
    K[~fin[faces].all(1)] = 0.0
    return K


def incidence(faces, V):
    """(face [3F], corner [3F], start [V], end [V]): the rows of the vertices, by ascending (vertex, face, corner)."""
    F = len(faces)
    key = (faces.reshape(-1).astype(np.int64) << 27) | (np.repeat(np.arange(F, dtype=np.int64), 3) << 2) | np.tile(np.arange(3), F)
    key.sort()
    v = key >> 27
    ar = np.arange(V)
    return (key >> 2) & ((1 << 25) - 1), key & 3, np.searchsorted(v, ar, "left"), np.searchsorted(v, ar, "right")


def initial_quadrics(u, fin, faces, V):
    """[V, 10]: per vertex the sum of its faces' quadrics in ascending face index, a fixed-order float64 sum from 0."""
    K = face_quadrics(u, fin, faces)
    inc_f, _, start, end = incidence(faces, V)
    Q = np.zeros((V, 10))
    deg = end - start
    for j in range(int(deg.max()) if V else 0):
        vs = np.flatnonzero(deg > j)
        Q[vs] = Q[vs] + K[inc_f[start[vs] + j]]
    return Q


def edges(faces):
    """(a [E], b [E], good [E]) of the sorted unique edges a < b; good: exactly two half-edges, of opposite direction."""
    a = faces.reshape(-1).astype(np.int64)
    b = faces[:, [1, 2, 0]].reshape(-1).astype(np.int64)
    key = (np.minimum(a, b) << 25) | (np.maximum(a, b) << 1) | (a > b)
    key.sort()
    pair = key >> 1
    head = np.flatnonzero(np.r_[True, pair[1:] != pair[:-1]])
    ln = np.diff(np.r_[head, len(key)])
    good = (ln == 2) & ((key[head] & 1) == 0) & ((key[np.minimum(head + 1, len(key) - 1)] & 1) == 1)
    return pair[head] >> 24, pair[head] & M24, good


def place(Qs, ua, ub, quadric):
    """(xbar [n, 3], cost [n], fell back to the midpoint [n]) of the summed quadrics Qs [n, 10] and the two ends' coordinates."""
    A, b, c = Qs[:, 0:6], Qs[:, 6:9], Qs[:, 9]
    m = (ua + ub) * 0.5
    d = ua - ub
    len2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    x = m.copy()
    fell = np.zeros(len(m), bool)
    if quadric:
        tr = (A[:, 0] + A[:, 3]) + A[:, 5]
        mu = (tr / 3.0) * 0.0009765625
        a00, a01, a02, a11, a12, a22 = A[:, 0] + mu, A[:, 1], A[:, 2], A[:, 3] + mu, A[:, 4], A[:, 5] + mu
        r0, r1, r2 = mu * m[:, 0] - b[:, 0], mu * m[:, 1] - b[:, 1], mu * m[:, 2] - b[:, 2]
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        det = (a00 * c00 + a01 * c01) + a02 * c02
        s = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                      ((c02 * r0 + c12 * r1) + c22 * r2) / det], 1)
        e = s - m
        dist2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        take = (tr > 0.0) & np.isfinite(s).all(1) & (dist2 <= len2)
        x[take] = s[take]
        fell = ~take
    ax0 = (A[:, 0] * x[:, 0] + A[:, 1] * x[:, 1]) + A[:, 2] * x[:, 2]
    ax1 = (A[:, 1] * x[:, 0] + A[:, 3] * x[:, 1]) + A[:, 4] * x[:, 2]
    ax2 = (A[:, 2] * x[:, 0] + A[:, 4] * x[:, 1]) + A[:, 5] * x[:, 2]
    xax = (x[:, 0] * ax0 + x[:, 1] * ax1) + x[:, 2] * ax2
    bx = (b[:, 0] * x[:, 0] + b[:, 1] * x[:, 1]) + b[:, 2] * x[:, 2]
    cost = (xax + 2.0 * bx) + c
    return x, np.where(cost > 0.0, cost, 0.0), fell


def _ring(faces, inc, e_idx, v, other):
    """The (edge, incident face) pairs of vertex v[i] of edge e_idx[i]: (edge [n], face [n], corner [n], next [n], prev [n],
    shared [n]: the face also holds other[i])."""
    inc_f, inc_c, start, end = inc
    deg = end[v] - start[v]
    rep = np.repeat(np.arange(len(v)), deg)
    ent = start[v][rep] + (np.arange(int(deg.sum())) - np.repeat(np.cumsum(deg) - deg, deg))
    f, c = inc_f[ent], inc_c[ent]
    nxt, prv = faces[f, (c + 1) % 3].astype(np.int64), faces[f, (c + 2) % 3].astype(np.int64)
    o = other[rep]
    return e_idx[rep], f, c, nxt, prv, (nxt == o) | (prv == o)


def candidates(u, fin, faces, Q, V, quadric):
    """One round's edges: dict of a, b [E], free [V], cand [E] bool, key [E] uint64 (NOKEY: no candidate), xbar [E, 3]."""
    ea, eb, good = edges(faces)
    E = len(ea)
    frozen = np.zeros(V, bool)
    frozen[ea[~good]] = True
    frozen[eb[~good]] = True
    frozen[ea[~fin[ea]]] = True
    frozen[eb[~fin[eb]]] = True
    free = ~frozen
    pre = np.flatnonzero(free[ea] & free[eb])
    inc = incidence(faces, V)
    assert E * V * V < 2 ** 62, "the reference's pair keys need E V^2 < 2^62"
    ra = _ring(faces, inc, pre, ea[pre], eb[pre])
    rb = _ring(faces, inc, pre, eb[pre], ea[pre])
    # the link condition: exactly two common neighbours ...
    common = np.bincount(ra[0][np.isin(ra[0] * V + ra[3], rb[0] * V + rb[3])], minlength=E)
    # ... and no ring edge opposite both ends
    oa, ob = ~ra[5], ~rb[5]
    ka = (ra[0][oa] * V + np.minimum(ra[3], ra[4])[oa]) * V + np.maximum(ra[3], ra[4])[oa]
    kb = (rb[0][ob] * V + np.minimum(rb[3], rb[4])[ob]) * V + np.maximum(rb[3], rb[4])[ob]
    clash = np.bincount(ra[0][oa][np.isin(ka, kb)], minlength=E) > 0
    xbar = np.zeros((E, 3))
    cost = np.zeros(E)
    fell = np.zeros(E, bool)
    xbar[pre], cost[pre], fell[pre] = place(Q[ea[pre]] + Q[eb[pre]], u[ea[pre]], u[eb[pre]], quadric)
    # no flip: every face at an end that does not hold both keeps a positive dot product of its old and its new normal
    flips = np.zeros(E, np.int64)
    for r in (ra, rb):
        keep = ~r[5]
        e, f, c = r[0][keep], r[1][keep], r[2][keep]
        p = u[faces[f]]                                     # [n, 3 corners, 3]
        n0 = _cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        p[np.arange(len(f)), c] = xbar[e]
        n1 = _cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        dot = (n0[0] * n1[0] + n0[1] * n1[1]) + n0[2] * n1[2]
        flips += np.bincount(e[~(dot > 0.0)], minlength=E)
    cand = np.zeros(E, bool)
    cand[pre] = True
    cand &= (common == 2) & ~clash & (flips == 0)
    bits = cost.astype(np.float32).view(np.uint32).astype(np.uint64)
    key = (bits << np.uint64(32)) | ((np.arange(E, dtype=np.uint64) * np.uint64(MULT)) & np.uint64(0xFFFFFFFF))
    key[~cand] = NOKEY
    on_edge = np.zeros(V, bool)
    on_edge[ea] = True
    on_edge[eb] = True
    link = (common == 2) & ~clash
    branches = {"links": int((~link[pre]).sum()), "flips": int((link & (flips > 0))[pre].sum()), "fallbacks": int((cand & fell).sum())}
    return {"a": ea, "b": eb, "free": free, "cand": cand, "key": key, "xbar": xbar, "frozen": int((on_edge & frozen).sum()),
            "branches": branches}


def select(c, V, passes):
    """sel [E] bool: `passes` passes of the two-ring minimum over the candidate keys."""
    ea, eb, cand, key = c["a"], c["b"], c["cand"], c["key"]
    blocked = np.zeros(V, bool)
    sel = np.zeros(len(ea), bool)
    for _ in range(passes):
        act = cand & ~blocked[ea] & ~blocked[eb]
        m1 = np.full(V, NOKEY, np.uint64)
        np.minimum.at(m1, ea[act], key[act])
        np.minimum.at(m1, eb[act], key[act])
        em = np.minimum(m1[ea], m1[eb])
        m2 = np.full(V, NOKEY, np.uint64)
        np.minimum.at(m2, ea, em)
        np.minimum.at(m2, eb, em)
        new = act & (key == m2[ea]) & (key == m2[eb])
        sel |= new
        end = np.zeros(V, bool)
        end[ea[new]] = True
        end[eb[new]] = True
        touch = end[ea] | end[eb]
        blocked[ea[touch]] = True
        blocked[eb[touch]] = True
    return sel


def _valid_faces(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    return f[ok]


def decimate(verts, faces, normals, colors, target, lo=LO, hi=HI, placement="quadric", passes=4, max_rounds=1024, trace=None):
    """((verts', faces', normals', colors' or None), stats): stats = dict(rounds, collapses [rounds], candidates [rounds], frozen,
    stopped).  trace: a list that receives per round (a [S], b [S], the faces before the round, the round's edges as `candidates`
    returns them with "trimmed": the trim dropped an edge)."""
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    V = len(v32)
    f_in = np.asarray(faces, np.int32).reshape(-1, 3)
    stats = {"rounds": 0, "collapses": [], "candidates": [], "frozen": 0, "stopped": "target"}
    if target >= len(f_in):
        return (v32, f_in, np.asarray(normals, np.float32), None if colors is None else np.asarray(colors, np.float32)), stats
    quadric = PLACEMENTS[placement]
    ctr, hs = box(lo, hi)
    pos = v32.copy()
    f = _valid_faces(f_in, V)
    with np.errstate(all="ignore"):
        fin = np.isfinite(pos).all(1)
        Q = initial_quadrics((pos.astype(np.float64) - ctr) / hs, fin, f, V)
        col = None if colors is None else np.asarray(colors, np.float32).reshape(-1, 3).astype(np.float64)
        cnt = np.ones(V, np.int64)
        while True:
            F = len(f)
            if F <= target:
                break
            if stats["rounds"] == max_rounds:
                stats["stopped"] = "max_rounds"
                break
            u = (pos.astype(np.float64) - ctr) / hs
            c = candidates(u, fin, f, Q, V, quadric)
            sel = select(c, V, passes)
            S_ = int(sel.sum())
            if F - 2 * S_ < target:                          # the trim: the smallest keys only
                k = (F - target + 1) // 2
                sel &= c["key"] <= np.sort(c["key"][sel])[k - 1]
            c["trimmed"] = int(sel.sum()) < S_
            a, b = c["a"][sel], c["b"][sel]
            if trace is not None:
                trace.append((a, b, f.copy(), c))
            if stats["rounds"] == 0:
                stats["frozen"] = c["frozen"]
            stats["rounds"] += 1
            stats["collapses"].append(len(a))
            stats["candidates"].append(int(c["cand"].sum()))
            if len(a) == 0:
                stats["stopped"] = "selected nothing"
                break
            pos[a] = (ctr + c["xbar"][sel] * hs).astype(np.float32)
            Q[a] = Q[a] + Q[b]
            cnt[a] = cnt[a] + cnt[b]
            if col is not None:
                col[a] = col[a] + col[b]
            remap = np.arange(V)
            remap[b] = a
            f = remap[f]
            f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
        used = np.zeros(V, bool)
        used[f.reshape(-1)] = True
        newid = np.cumsum(used) - 1
        vo = pos[used]
        fo = newid[f].astype(np.int32).reshape(-1, 3)
        co = None if col is None else (col / cnt.astype(np.float64)[:, None]).astype(np.float32)[used]
        no = SM.normals(vo, SM.entries(fo, len(vo)), *SM.box(lo, hi))
    return (vo, fo, no, co), stats


# ------------------------------------------------------------------------------------------------ measures of a mesh
def euler(faces):
    """V - E + F over the referenced vertices."""
    a, _, _ = edges(np.asarray(faces))
    return len(np.unique(faces)) - len(a) + len(faces)


def all_edges_paired(faces):
    return bool(edges(np.asarray(faces))[2].all())


def boundary_vertices(faces):
    a, b, good = edges(np.asarray(faces))
    return np.unique(np.r_[a[~good], b[~good]])


# ------------------------------------------------------------------------------------------------ the shared meshes
@functools.lru_cache(maxsize=None)
def mesh(name):
    """(verts, faces, normals, colors): sphere, box, plate and noise of tests/_simplify_ref.py, `half` (the faces of the sphere
    with a corner above z = 0.05: an open mesh), `junk` (the sphere with NaN / +-inf coordinates, indices outside [0, V) and a
    face with two equal corners) and `big` (the sphere at R = 128, 55 612 faces)."""
    if name in ("sphere", "box", "plate", "noise"):
        return S.mesh(name)
    if name == "big":
        vol = S.M.lattice_points(128, LO, HI).astype(np.float64)
        vol = (0.6 - np.linalg.norm(vol - [0.1, -0.05, 0.05], axis=1)).reshape(128, 128, 128).astype(np.float32)
        v, f, n = S.M.marching_cubes(vol, 0.0, LO, HI)
        out = (v, f, n, (0.5 + 0.5 * np.sin(3.0 * v.astype(np.float64))).astype(np.float32))
    else:
        v, f, n, c = (np.array(x) for x in S.mesh("sphere"))
        if name == "half":
            f = f[(v[f][:, :, 2] > 0.05).any(1)]
        elif name == "junk":
            v[5], v[70, 1], v[300, 2], v[301, 0] = np.nan, np.inf, -np.inf, np.nan
            f[11, 0], f[12, 2], f[13, 1], f[14, 1] = -1, len(v), 2 ** 31 - 1, f[14, 0]
        else:
            raise KeyError(name)
        out = (v, f, n, c)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name, target, placement="quadric", with_colors=True, passes=4):
    v, f, n, c = mesh(name)
    trace = []
    out, stats = decimate(v, f, n, c if with_colors else None, target, LO, HI, placement, passes, trace=trace)
    return out, stats, trace
