"""numpy reference of mesh extraction (include/nerf_hip.h "mesh extraction"): the lattice, marching cubes
over a density volume with the generated case table (csrc/gen_mc_table.py), float32 in the kernels' operation order, and the
mesh checks the tests share (closed, oriented, Euler characteristic, enclosed volume)."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc")
_F = np.float32


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(CSRC, "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = load_generator()
TABLE = GEN.table()                                             # [256] lists of (e0, e1, e2)
NTRI = np.array([len(r) for r in TABLE], dtype=np.int64)
TRI = np.zeros((256, GEN.MAX_TRIS, 3), dtype=np.int64)
for _s, _r in enumerate(TABLE):
    if _r:
        TRI[_s, :len(_r)] = np.array(_r)
EDGE_CORNER = np.array(GEN.EDGE_CORNER)
EDGE_AXIS = np.array(GEN.EDGE_AXIS)
CORNER_OFF = np.array([[c & 1, (c >> 1) & 1, c >> 2] for c in range(8)])     # (dx, dy, dz)


def spacing(R, lo, hi):
    """h_a = (hi_a - lo_a) / R, float32, two roundings."""
    lo, hi = np.asarray(lo, _F), np.asarray(hi, _F)
    return (hi - lo) / _F(R)


def axis_coords(R, lo, hi):
    """[3, R] float32: p_a(i) = lo_a + ((float)i + 0.5f) * h_a."""
    lo = np.asarray(lo, _F)
    h = spacing(R, lo, hi)
    i = np.arange(R, dtype=_F) + _F(0.5)
    return np.stack([lo[a] + i * h[a] for a in range(3)])


def lattice_points(R, lo, hi):
    """[R^3, 3] float32 positions in linear order i + R (j + R k)."""
    p = axis_coords(R, lo, hi)
    k, j, i = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
    return np.stack([p[0][i], p[1][j], p[2][k]], -1).reshape(-1, 3)


def gradient(v, h):
    """[R, R, R, 3] float32 central differences (v[+1] - v[-1]) / (2 h_a), one-sided (v[1] - v[0]) / h_a at the border."""
    R = v.shape[0]
    g = np.empty(v.shape + (3,), _F)
    for a in range(3):
        ax = 2 - a                                               # vol[k, j, i]: x is the last array axis
        va = np.moveaxis(v, ax, 0)
        ga = np.empty_like(va)
        ga[1:-1] = (va[2:] - va[:-2]) / (_F(2) * h[a])
        ga[0] = (va[1] - va[0]) / h[a]
        ga[R - 1] = (va[R - 1] - va[R - 2]) / h[a]
        g[..., a] = np.moveaxis(ga, 0, ax)
    return g


def marching_cubes(vol, iso, lo, hi):
    """(verts [V, 3] f32, faces [F, 3] int32, normals [V, 3] f32) of the semantics in include/nerf_hip.h."""
    v = np.ascontiguousarray(vol, dtype=_F)
    R = v.shape[0]
    iso = _F(iso)
    h = spacing(R, lo, hi)
    p = axis_coords(R, lo, hi)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        inside = v > iso
        g = gradient(v, h)
        cross = np.zeros((3,) + v.shape, bool)                   # cross[a][k, j, i]: edge (q, a) carries a vertex
        cross[0][:, :, :-1] = inside[:, :, :-1] != inside[:, :, 1:]
        cross[1][:, :-1, :] = inside[:, :-1, :] != inside[:, 1:, :]
        cross[2][:-1, :, :] = inside[:-1, :, :] != inside[1:, :, :]
        cnt = cross.sum(0).reshape(-1)
        base = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
        V = int(cnt.sum())
        vid = np.full((3, R ** 3), -1, np.int64)
        rank = np.zeros(R ** 3, np.int64)
        for a in range(3):
            c = cross[a].reshape(-1)
            vid[a][c] = base[c] + rank[c]
            rank += c
        verts = np.zeros((V, 3), _F)
        normals = np.zeros((V, 3), _F)
        for a in range(3):
            kk, jj, ii = np.nonzero(cross[a])
            q = np.stack([ii, jj, kk], 1)
            q1 = q.copy()
            q1[:, a] += 1
            v0, v1 = v[kk, jj, ii], v[q1[:, 2], q1[:, 1], q1[:, 0]]
            t = (iso - v0) / (v1 - v0)
            t = np.where(np.isnan(t), _F(0.5), np.minimum(np.maximum(t, _F(0)), _F(1))).astype(_F)
            ids = vid[a][ii + R * (jj + R * kk)]
            pos = np.stack([p[0][ii], p[1][jj], p[2][kk]], 1)
            pos[:, a] = pos[:, a] + t * h[a]
            verts[ids] = pos
            g0, g1 = g[kk, jj, ii], g[q1[:, 2], q1[:, 1], q1[:, 0]]
            gv = g0 + t[:, None] * (g1 - g0)
            ng = np.sqrt((gv[:, 0] * gv[:, 0] + gv[:, 1] * gv[:, 1]) + gv[:, 2] * gv[:, 2])
            ok = np.isfinite(ng) & (ng > 0)
            n = np.where(ok[:, None], -(gv / np.where(ok, ng, _F(1))[:, None]), _F(0)).astype(_F)
            normals[ids] = n
    # faces: cells (i, j, k < R - 1) in linear order, then table order
    ins = inside.astype(np.int64)
    case = np.zeros((R - 1,) * 3, np.int64)
    for c in range(8):
        dx, dy, dz = CORNER_OFF[c]
        case += ins[dz:dz + R - 1, dy:dy + R - 1, dx:dx + R - 1] << c
    nt = NTRI[case]
    kk, jj, ii = np.nonzero(nt)
    cs = case[kk, jj, ii]
    eid = np.zeros((len(cs), 12), np.int64)
    for e in range(12):
        dx, dy, dz = CORNER_OFF[EDGE_CORNER[e]]
        eid[:, e] = vid[EDGE_AXIS[e]][(ii + dx) + R * ((jj + dy) + R * (kk + dz))]
    tri = TRI[cs]                                                # [cells, MAX_TRIS, 3] edge ids
    fv = np.take_along_axis(eid[:, None, :].repeat(GEN.MAX_TRIS, 1), tri, axis=2)
    keep = np.arange(GEN.MAX_TRIS)[None, :] < nt[kk, jj, ii][:, None]
    faces = fv[keep].reshape(-1, 3)
    assert (faces >= 0).all()
    return verts, faces.astype(np.int32), normals


# ------------------------------------------------------------------------------------------------ mesh checks
def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def closed_and_oriented(faces):
    """Every directed edge exactly once and its reverse present: every undirected edge in exactly two faces, consistently."""
    d = directed_edges(faces)
    if len(d) == 0:
        return True
    m = int(d.max()) + 1
    key = d[:, 0] * m + d[:, 1]
    rev = d[:, 1] * m + d[:, 0]
    if len(np.unique(key)) != len(key):
        return False
    return bool(np.isin(rev, key).all())


def undirected_edge_counts(faces):
    d = np.sort(directed_edges(faces), 1)
    _, c = np.unique(d[:, 0] * (int(d.max()) + 1) + d[:, 1], return_counts=True)
    return c


def euler(verts, faces):
    """V - E + F over the vertices the faces use."""
    d = np.sort(directed_edges(faces), 1)
    E = len(np.unique(d[:, 0] * (int(d.max()) + 1) + d[:, 1])) if len(d) else 0
    return len(np.unique(np.asarray(faces))) - E + len(faces)


def enclosed_volume(verts, faces):
    """Divergence theorem: sum of a . (b x c) / 6 in float64 (positive for outward-oriented closed meshes)."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def boxes_union(boxes):
    """(volume, surface area) of a union of axis-aligned boxes [(centre, half-size), ...], exact on the boxes' own grid."""
    lo = np.array([np.subtract(c, h) for c, h in boxes], np.float64)
    hi = np.array([np.add(c, h) for c, h in boxes], np.float64)
    xs = [np.unique(np.concatenate([lo[:, a], hi[:, a]])) for a in range(3)]
    mids = [0.5 * (x[1:] + x[:-1]) for x in xs]
    M = np.stack(np.meshgrid(*mids, indexing="ij"), -1)
    occ = np.zeros(M.shape[:3], bool)
    for l, u in zip(lo, hi):
        occ |= ((M > l) & (M < u)).all(-1)
    w = [np.diff(x) for x in xs]
    vol = float((occ * w[0][:, None, None] * w[1][None, :, None] * w[2][None, None, :]).sum())
    area = 0.0
    for a in range(3):
        o = np.moveaxis(np.pad(occ, [(1, 1) if b == a else (0, 0) for b in range(3)]), a, 0)
        flips = o[1:] != o[:-1]
        others = [w[b] for b in range(3) if b != a]
        area += float((flips.sum(0) * others[0][:, None] * others[1][None, :]).sum())
    return vol, area

