"""numpy reference of include/nerf_hip.h "texture atlas" (a helper module, not a test): the layout in Python integers, rows, store,
UVs and sampler in float32 arrays, operator for operator in the header's order.  numpy rounds every float32 operation on its own
(no fused multiply-add), as the library does with -ffp-contract=off; its division and square root are correctly rounded."""
import math

import numpy as np

MAX_SIDE, MAX_FACES, MIN_TEXELS, MAX_TEXELS = 16384, 1 << 24, 2, 64
f32 = np.float32


def layout(F, T):
    """(W, H, C, S), or None where the library refuses."""
    if not (0 <= F <= MAX_FACES and MIN_TEXELS <= T <= MAX_TEXELS):
        return None
    cells = (F + 1) // 2
    C = max(1, math.isqrt(cells))
    if C * C < cells:
        C += 1
    S = T + 2
    W, H = C * S, max(1, -(-cells // C)) * S
    return None if max(W, H) > MAX_SIDE else (W, H, C, S)


def owner(lay, X, Y):
    """(face, i, j) of the atlas texels (X, Y) (integer arrays): the local texel is mirrored for the odd face."""
    _, _, C, S = lay
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    c = (Y // S) * C + X // S
    i, j = X % S, Y % S
    odd = i + j > S - 1
    return 2 * c + odd, np.where(odd, S - 1 - i, i), np.where(odd, S - 1 - j, j)


def place(lay, f, i, j):
    """(X, Y) of the local texels (i, j) of the faces f."""
    _, _, C, S = lay
    f, i, j = (np.asarray(a, np.int64) for a in (f, i, j))
    c, odd = f >> 1, (f & 1) == 1
    return (c % C) * S + np.where(odd, S - 1 - i, i), (c // C) * S + np.where(odd, S - 1 - j, j)


def _pos(x):
    return np.where(x > 0, x, f32(0))                   # NaN -> 0


def _unit(x):
    x = _pos(x)
    return np.where(x < 1, x, f32(1)).astype(f32)


def _good(faces, f, V):
    """(ok [n], corners [n, 3] with 0 where not ok) of the faces f: inside [0, F) with every index inside [0, V)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    f = np.asarray(f, np.int64)
    ok = (f >= 0) & (f < len(faces))
    g = faces[np.where(ok, f, 0)] if len(faces) else np.zeros((len(f), 3), np.int64)
    ok = ok & ((g >= 0) & (g < V)).all(1)
    return ok, np.where(ok[:, None], g, 0)


def _rows(verts, normals, g, ok, wb, wc):
    v, nr = np.asarray(verts, f32).reshape(-1, 3), np.asarray(normals, f32).reshape(-1, 3)
    rows = np.zeros((len(ok), 11), f32)
    if not len(v) or not ok.any():
        return rows
    with np.errstate(all="ignore"):
        wb, wc = wb.astype(f32)[:, None], wc.astype(f32)[:, None]
        wa = (f32(1) - wb) - wc
        A, B, C = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
        x = (wa * A + wb * B) + wc * C
        pa, pb, pc = (_pos(w).astype(f32) for w in (wa, wb, wc))
        m = (pa * nr[g[:, 0]] + pb * nr[g[:, 1]]) + pc * nr[g[:, 2]]
        ln = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        fine = (ln > 0) & (ln <= np.finfo(f32).max)
        n = np.where(fine[:, None], m / np.where(fine, ln, f32(1))[:, None], f32(0)).astype(f32)
    assert x.dtype == f32 and m.dtype == f32 and ln.dtype == f32
    full = np.zeros_like(rows)
    full[:, 0:3], full[:, 3:6], full[:, 8:11] = x, -n, -n
    rows[ok] = full[ok]
    return rows


def texel_rows(verts, normals, faces, T, p0=0, count=None):
    """float32 [count, 11]: the query rows of the atlas texels [p0, p0 + count)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    lay = layout(len(faces), T)
    W, H = lay[:2]
    p = np.arange(p0, W * H if count is None else p0 + count, dtype=np.int64)
    f, i, j = owner(lay, p % W, p // W)
    ok, g = _good(faces, np.where(f < len(faces), f, -1), len(np.asarray(verts).reshape(-1, 3)))
    d = f32(T - 1)
    return _rows(verts, normals, g, ok, i.astype(f32) / d, j.astype(f32) / d)


def store(raw, faces, V, T):
    """uint8 [H, W, 3] of raw [W H, 4] (all texels)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    lay = layout(len(faces), T)
    W, H = lay[:2]
    p = np.arange(W * H, dtype=np.int64)
    f = owner(lay, p % W, p // W)[0]
    ok, _ = _good(faces, np.where(f < len(faces), f, -1), V)
    with np.errstate(all="ignore"):
        b = np.rint(f32(255) * _unit(np.asarray(raw, f32).reshape(-1, 4)[:, :3])).astype(np.uint8)
    return np.where(ok[:, None], b, 0).astype(np.uint8).reshape(H, W, 3)


def uvs(F, T):
    """float32 [F, 3, 2]."""
    lay = layout(F, T)
    W, H = lay[:2]
    f = np.repeat(np.arange(F, dtype=np.int64), 3)
    X, Y = place(lay, f, np.tile([0, T - 1, 0], F), np.tile([0, 0, T - 1], F))
    u = (X.astype(f32) + f32(0.5)) / f32(W)
    v = f32(1) - (Y.astype(f32) + f32(0.5)) / f32(H)
    return np.stack([u, v], 1).astype(f32).reshape(F, 3, 2)


def clamp_bary(bary):
    b = np.asarray(bary, f32).reshape(-1, 2)
    wb = _unit(b[:, 0])
    hi = f32(1) - wb
    wc = _pos(b[:, 1]).astype(f32)
    return wb, np.where(wc < hi, wc, hi).astype(f32)


def footprint(lay, T, f, wb, wc):
    """(X [n, 4], Y [n, 4], w [n, 4]) of the bilinear lookups of faces f at the clamped barycentrics, in the order 00, 10, 01, 11."""
    S = lay[3]
    d = f32(T - 1)
    x, y = wb * d, wc * d
    i0 = np.clip(np.floor(x).astype(np.int64), 0, S - 2)
    j0 = np.clip(np.floor(y).astype(np.int64), 0, S - 2)
    fx, fy = x - i0.astype(f32), y - j0.astype(f32)
    gx, gy = f32(1) - fx, f32(1) - fy
    w = np.stack([gx * gy, fx * gy, gx * fy, fx * fy], 1)
    assert w.dtype == f32
    X, Y = place(lay, f[:, None], i0[:, None] + np.array([0, 1, 0, 1]), j0[:, None] + np.array([0, 0, 1, 1]))
    return X, Y, w


def sample(image, verts, normals, faces, T, sface, bary, rows=False):
    """rgb float32 [n, 3] (and rows [n, 11])."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(faces)
    lay = layout(F, T)
    sface = np.asarray(sface, np.int64)
    wb, wc = clamp_bary(bary)
    inside = (sface >= 0) & (sface < F)
    X, Y, w = footprint(lay, T, np.where(inside, sface, 0), wb, wc)
    c = np.asarray(image, np.uint8)[Y, X].astype(f32) / f32(255)            # [n, 4, 3]
    rgb = ((w[:, 0, None] * c[:, 0] + w[:, 1, None] * c[:, 1]) + w[:, 2, None] * c[:, 2]) + w[:, 3, None] * c[:, 3]
    assert rgb.dtype == f32
    rgb = np.where(inside[:, None], rgb, f32(0)).astype(f32)
    if not rows:
        return rgb
    ok, g = _good(faces, sface, len(np.asarray(verts).reshape(-1, 3)))
    return rgb, _rows(verts, normals, g, ok, wb, wc)


def bake(query, verts, normals, faces, T):
    """(image, uv) with query(rows [n, 11]) -> raw [n, 4] in numpy."""
    rows = texel_rows(verts, normals, faces, T)
    V = len(np.asarray(verts).reshape(-1, 3))
    return store(query(rows), faces, V, T), uvs(len(np.asarray(faces).reshape(-1, 3)), T)


def vertex_normals(verts, faces):
    """float32 [V, 3] unit normals (area-weighted, plain float64): inputs for the tests, not part of the rule."""
    v, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v)
    for c in range(3):
        np.add.at(n, f[:, c], fn)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0).astype(f32)
