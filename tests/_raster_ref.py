"""The mesh rasteriser of include/nerf_hip.h "mesh rendering" in numpy (a helper module, not a test): float32 arrays for the float
steps, one rounding per operation in the header's order; int64 for the snapped coordinates and the edge functions; the key
minimum by np.minimum.at.  Same outputs and the same stats as csrc/raster.hip, bit for bit."""
import numpy as np

from tests import _camera_ref as C
from tests._camera_ref import intrinsics, project, view_of  # noqa: F401  (the camera; the names the tests use)

F32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
SNAP = 256
GUARD = F32(2.0 ** 20)
OK, DROP_DEPTH, DROP_OTHER = 0, 1, 2
SMALL_MAX = 16                                                          # NERF_RASTER_SMALL_MAX


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """_camera_ref.look_at with y up by default, for which its fallback for a vertical view changes nothing."""
    return C.look_at(eye, target, up)


def area2(X, Y):
    """D int64: (Xb - Xa)(Yc - Ya) - (Yb - Ya)(Xc - Xa)."""
    return (X[..., 1] - X[..., 0]) * (Y[..., 2] - Y[..., 0]) - (Y[..., 1] - Y[..., 0]) * (X[..., 2] - X[..., 0])


def setup(verts, faces, view, near, cull=False):
    """why [F] (OK / DROP_DEPTH / DROP_OTHER), X, Y int64 [F, 3], z float32 [F, 3], s int64 [F] (valid where why == OK)."""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V, Fn = len(verts), len(f)
    why = np.full(Fn, OK, np.int64)
    X, Y = np.zeros((Fn, 3), np.int64), np.zeros((Fn, 3), np.int64)
    z = np.zeros((Fn, 3), F32)
    s = np.zeros(Fn, np.int64)
    inside = ((f >= 0) & (f < V)).all(1)
    why[~inside] = DROP_OTHER
    g = np.where(inside[:, None], f, 0)
    if V == 0:
        return why, X, Y, z, s
    p = verts[g]                                                        # [F, 3, 3]
    finite = np.isfinite(p).all((1, 2))
    why[inside & ~finite] = DROP_OTHER
    u, v, zc = (a.reshape(Fn, 3) for a in project(p.reshape(-1, 3), view))
    with np.errstate(invalid="ignore"):
        seen = ((zc >= F32(near)) & (zc <= np.finfo(F32).max)).all(1)
        band = ((np.abs(u) <= GUARD) & (np.abs(v) <= GUARD)).all(1)
    live = why == OK
    why[live & ~(seen & band)] = DROP_DEPTH
    live = why == OK
    with np.errstate(invalid="ignore"):
        X[live] = np.rint(u[live] * F32(SNAP)).astype(np.int64)
        Y[live] = np.rint(v[live] * F32(SNAP)).astype(np.int64)
    z[live] = zc[live]
    D = area2(X, Y)
    why[live & ((D == 0) | (bool(cull) & (D > 0)))] = DROP_OTHER
    s[:] = np.where(D > 0, 1, -1)
    return why, X, Y, z, s


def _edge(Ux, Uy, Vx, Vy, Px, Py):
    return (Vx - Ux) * (Py - Uy) - (Vy - Uy) * (Px - Ux)


def pixel(X, Y, z, s, px, py):
    """(covered, wb, wc, depth) at the pixel centres (px, py); X, Y, z [..., 3] and s broadcast against them."""
    Px, Py = SNAP * np.asarray(px, np.int64), SNAP * np.asarray(py, np.int64)
    Ea = s * _edge(X[..., 1], Y[..., 1], X[..., 2], Y[..., 2], Px, Py)
    Eb = s * _edge(X[..., 2], Y[..., 2], X[..., 0], Y[..., 0], Px, Py)
    Ec = s * _edge(X[..., 0], Y[..., 0], X[..., 1], Y[..., 1], Px, Py)
    cov = (Ea >= 0) & (Eb >= 0) & (Ec >= 0)
    with np.errstate(all="ignore"):
        qa, qb, qc = Ea.astype(F32) / z[..., 0], Eb.astype(F32) / z[..., 1], Ec.astype(F32) / z[..., 2]
        Q = (qa + qb) + qc
        wb, wc = qb / Q, qc / Q
        d = ((Ea + Eb) + Ec).astype(F32) / Q
    return cov, wb.astype(F32), wc.astype(F32), d.astype(F32)


def boxes(X, Y, H, W):
    """(x0, x1, y0, y1) int64 [F]: the pixels with X_min <= 256 px <= X_max, Y_min <= 256 py <= Y_max, clipped to the image."""
    x0 = np.maximum((X.min(1) + (SNAP - 1)) >> 8, 0)
    x1 = np.minimum(X.max(1) >> 8, W - 1)
    y0 = np.maximum((Y.min(1) + (SNAP - 1)) >> 8, 0)
    y1 = np.minimum(Y.max(1) >> 8, H - 1)
    return x0, x1, y0, y1


def clear(H, W):
    return np.full(H * W, EMPTY, np.uint64), np.zeros(4, np.uint64)


def keys_of(depth, ids):
    return (np.ascontiguousarray(depth, F32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(ids, np.uint64)


def draw(keys, stats, verts, faces, view, H, W, near, cull=False, face_base=0):
    """nerf_raster_draw into keys [H W] uint64 and stats [4] uint64, in place."""
    why, X, Y, z, s = setup(verts, faces, view, near, cull)
    stats[0] += np.uint64((why == OK).sum())
    stats[1] += np.uint64((why == DROP_DEPTH).sum())
    stats[2] += np.uint64((why == DROP_OTHER).sum())
    x0, x1, y0, y1 = boxes(X, Y, H, W)
    for k in np.nonzero((why == OK) & (x0 <= x1) & (y0 <= y1))[0]:
        py, px = np.mgrid[y0[k]:y1[k] + 1, x0[k]:x1[k] + 1]
        cov, _, _, d = pixel(X[k], Y[k], z[k], s[k], px, py)
        if cov.any():
            np.minimum.at(keys, (py * W + px)[cov], keys_of(d[cov], np.full(int(cov.sum()), face_base + k)))
            stats[3] += np.uint64(cov.sum())
    return keys, stats


def resolve(keys, verts, faces, view, H, W, near):
    """(face [H W] int32, bary [H W, 2], depth [H W], acc [H W]) float32."""
    n = H * W
    face, bary = np.full(n, -1, np.int32), np.zeros((n, 2), F32)
    depth, acc = np.zeros(n, F32), np.zeros(n, F32)
    ids = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    Fn = len(np.asarray(faces).reshape(-1, 3))
    cand = np.nonzero((keys != EMPTY) & (ids < Fn))[0]
    if len(cand) == 0:
        return face, bary, depth, acc
    why, X, Y, z, s = setup(verts, faces, view, near, False)
    k = ids[cand]
    cov, wb, wc, d = pixel(X[k], Y[k], z[k], s[k], cand % W, cand // W)
    ok = cov & (why[k] == OK)
    p = cand[ok]
    face[p], bary[p, 0], bary[p, 1], depth[p], acc[p] = k[ok], wb[ok], wc[ok], d[ok], 1.0
    return face, bary, depth, acc


def shade(face, bary, faces, V, background, colors=None, rgb_in=None):
    """rgb [H W, 3] float32; background [3] or [H W, 3]."""
    n = len(face)
    out = np.broadcast_to(np.asarray(background, F32).reshape(-1, 3), (n, 3)).copy()
    hit = face >= 0
    if rgb_in is not None:
        out[hit] = np.asarray(rgb_in, F32).reshape(n, 3)[hit]
        return out
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    hit &= face < len(f)
    g = f[np.where(hit, face, 0)] if len(f) else np.zeros((n, 3), np.int64)
    hit &= ((g >= 0) & (g < V)).all(1)
    g = g[hit]
    c = np.asarray(colors, F32).reshape(-1, 3)
    wb, wc = bary[hit, 0:1], bary[hit, 1:2]
    wa = (F32(1.0) - wb) - wc
    out[hit] = (wa * c[g[:, 0]] + wb * c[g[:, 1]]) + wc * c[g[:, 2]]
    return out


def render(verts, faces, view, H, W, near, cull=False):
    """keys, stats, face, bary, depth, acc of one cleared draw."""
    keys, stats = clear(H, W)
    draw(keys, stats, verts, faces, view, H, W, near, cull)
    return (keys, stats) + resolve(keys, verts, faces, view, H, W, near)


# ------------------------------------------------------------------------------------------------ shared test scenes
def from_camera(c2w, xc, yc, zc):
    """The world point (float64) at camera coordinates (xc, yc) and depth zc."""
    c = np.asarray(c2w, np.float64)[:3, :4]
    return c[:, :3] @ np.array([xc, yc, -zc], np.float64) + c[:, 3]


def from_pixel(c2w, K, u, v, zc):
    """The world point whose projection is (u, v) at depth zc, up to float rounding."""
    K = np.asarray(K, np.float64)
    return from_camera(c2w, (u - K[0, 2]) / K[0, 0] * zc, (K[1, 2] - v) / K[1, 1] * zc, zc)


def quad(c2w, K, corners, depths):
    """(verts [4, 3] float32, faces [2, 3] int32): the quad with screen corners [(u, v)] * 4 (in order around it) at the given
    depths, as the triangles (0, 1, 2) and (0, 2, 3)."""
    v = np.array([from_pixel(c2w, K, u, w, z) for (u, w), z in zip(corners, depths)], F32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def fan(c2w, K, sizes, margin=0.3):
    """Right triangles in front of the camera, one per (x0, y0, w, h): the bounding box of its snapped corners is the pixels
    [x0, x0 + w) x [y0, y0 + h) (the corners lie `margin` of a pixel outside the outermost pixel centres), before clipping to
    the image; depths differ from face to face."""
    verts, faces = [], []
    for k, (x0, y0, w, h) in enumerate(sizes):
        z = 2.0 + 0.01 * k
        a, b = x0 - margin, y0 - margin
        c, d = x0 + w - 1 + margin, y0 + h - 1 + margin
        verts += [from_pixel(c2w, K, a, b, z), from_pixel(c2w, K, c, b, z + 0.2), from_pixel(c2w, K, a, d, z + 0.1)]
        faces.append([3 * k, 3 * k + 1 + (k % 2), 3 * k + 2 - (k % 2)])                  # both windings
    return np.array(verts, F32), np.array(faces, np.int32)


def drop_scene(c2w, verts, faces, near):
    """`faces` (at least 20) over `verts` with ten of them replaced by faces the rule drops; (verts', faces', depth or guard band,
    other).  Extra vertices: e0 NaN, e1 behind the camera, e2 between the camera and near, e3 outside the guard band, e4 +inf."""
    v = np.asarray(verts, F32)
    V = len(v)
    extra = np.array([[np.nan, 0.0, 0.0], from_camera(c2w, 0.1, 0.1, -1.0), from_camera(c2w, 0.0, 0.1, 0.5 * near),
                      from_camera(c2w, 3.0e6 * near, 0.0, 1.5 * near), [np.inf, 0.0, 0.0]], np.float64).astype(F32)
    v = np.concatenate([v, extra])
    f = np.array(faces, np.int32).copy()
    a, b = int(f[0, 0]), int(f[0, 1])
    big = np.iinfo(np.int32)
    f[1] = [a, b, V + 2]                                                  # straddles near: depth
    f[3] = [V + 1, a, b]                                                  # a vertex behind the camera: depth
    f[5] = [a, V + 3, b]                                                  # guard band: depth
    f[7] = [a, a, b]                                                      # zero area: other
    f[9] = [V, b, a]                                                      # NaN vertex: other
    f[11] = [a, b, V + 5]                                                 # index V' (one past the end): other
    f[13] = [-1, a, b]
    f[15] = [a, big.max, b]
    f[17] = [a, b, big.min]
    f[len(f) - 1] = [V + 4, a, b]                                         # infinite vertex: other (the last face, in a partial wave)
    return v, f, 3, 7
