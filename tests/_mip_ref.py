"""numpy reference of include/nerf_hip.h "texture mip pyramid" (a helper module, not a test): the levels in Python integers, the
reduce, the level of detail and the trilinear lookup in float32 arrays, operator for operator in the header's order, on the layout,
owner, place and sampler clamps of tests/_texture_ref.py and the snapped faces of tests/_raster_ref.py.  numpy rounds every float32
operation on its own; its division and square root are correctly rounded.  Same bits as csrc/mip.hip."""
import numpy as np

from tests import _raster_ref as R
from tests import _texture_ref as T

MAX_LEVELS = 6                                                          # NERF_MIP_MAX_LEVELS
f32 = np.float32


def levels(texels):
    """(T_0, ..., T_{L-1}), or None where the library refuses."""
    if not T.MIN_TEXELS <= texels <= T.MAX_TEXELS:
        return None
    out = [int(texels)]
    while out[-1] > 2:
        out.append((out[-1] + 1) // 2)
    assert len(out) <= MAX_LEVELS
    return tuple(out)


def lookup(image, lay, f, x, y, reads=None):
    """float32 [n, 3]: the bilinear lookup of "texture atlas" at the local texel coordinates (x, y) float32 [n] of the faces f.
    reads: a list that takes (X [n, 4], Y [n, 4], w [n, 4]): the texels read and their weights."""
    S = lay[3]
    f = np.asarray(f, np.int64)
    i0 = np.clip(np.floor(x).astype(np.int64), 0, S - 2)
    j0 = np.clip(np.floor(y).astype(np.int64), 0, S - 2)
    fx, fy = x - i0.astype(f32), y - j0.astype(f32)
    gx, gy = f32(1) - fx, f32(1) - fy
    w = np.stack([gx * gy, fx * gy, gx * fy, fx * fy], 1)
    X, Y = T.place(lay, f[:, None], i0[:, None] + np.array([0, 1, 0, 1]), j0[:, None] + np.array([0, 0, 1, 1]))
    if reads is not None:
        reads.append((X, Y, w))
    c = np.asarray(image, np.uint8)[Y, X].astype(f32) / f32(255)         # [n, 4, 3]
    rgb = ((w[:, 0, None] * c[:, 0] + w[:, 1, None] * c[:, 1]) + w[:, 2, None] * c[:, 2]) + w[:, 3, None] * c[:, 3]
    assert rgb.dtype == f32 and w.dtype == f32
    return rgb


def _inner(fine, lf, Tf, Tc, f, i, j, reads=None):
    """int64 [n, 3]: the bytes of the in-triangle texels (i, j), i + j <= Tc - 1, of the faces f.  reads: a list that takes
    (k [m], X [m, 4], Y [m, 4], w [m, 4]), the positions k in f of the lanes that looked up, the fine texels they read and the
    weights."""
    top, den = f32(Tf - 1), f32(Tc - 1)
    x = (i * (Tf - 1)).astype(f32) / den
    y = (j * (Tf - 1)).astype(f32) / den
    d = f32(0.25) * (top / den)
    assert x.dtype == f32 and np.asarray(d).dtype == f32
    every = np.arange(len(f))

    def look(k, xs, ys):
        got = []
        rgb = lookup(fine, lf, f[k], xs, ys, got if reads is not None else None)
        if reads is not None:
            reads.append((k,) + got[0])
        return rgb
    c = look(every, x, y)
    zero = f32(0)
    pairs = []
    for ox, oy in ((d, zero), (zero, d), (d, d), (d, zero - d)):
        ax, ay, bx, by = x + ox, y + oy, x - ox, y - oy
        both = (ax >= 0) & (ay >= 0) & (ax + ay <= top) & (bx >= 0) & (by >= 0) & (bx + by <= top)
        p = c + c
        k = np.nonzero(both)[0]
        if len(k):
            p[k] = look(k, ax[k], ay[k]) + look(k, bx[k], by[k])
        pairs.append(p)
    value = ((pairs[0] + pairs[1]) + (pairs[2] + pairs[3])) * f32(0.125)
    assert value.dtype == f32
    return np.rint(f32(255) * T._unit(value)).astype(np.int64)


def _texel(fine, lf, Tf, Tc, f, i, j, reads=None, who=None):
    """int64 [n, 3]: the bytes of the local texels (i, j) of the faces f of the coarse level, in-triangle or gutter.  who [n]: the
    coarse texel on whose behalf the lane works, handed down to `reads` in place of its position."""
    n = len(f)
    who = np.arange(n) if who is None else who
    out = np.zeros((n, 3), np.int64)
    s = i + j
    m = np.nonzero(s <= Tc - 1)[0]
    if len(m):
        got = [] if reads is not None else None
        out[m] = _inner(fine, lf, Tf, Tc, f[m], i[m], j[m], got)
        if reads is not None:
            reads.extend((who[m][k], X, Y, w) for k, X, Y, w in got)
    g = np.nonzero(s > Tc - 1)[0]
    if len(g):
        ff, ii, jj, ww = f[g], i[g], j[g], who[g]
        leg = (ii == 0) | (jj == 0)
        di = np.where(jj == 0, 1, 0)
        dj = 1 - di

        def v(a, b):
            return _texel(fine, lf, Tf, Tc, ff, a, b, reads, ww)
        # on a leg: 2 v(one step back) - v(two steps back); elsewhere v(i - 1, j) + v(i, j - 1) - v(i - 1, j - 1)
        A = v(np.where(leg, ii - di, ii - 1), np.where(leg, jj - dj, jj))
        B = v(np.where(leg, ii - 2 * di, ii), np.where(leg, jj - 2 * dj, jj - 1))
        Cc = v(np.where(leg, ii - di, ii - 1), np.where(leg, jj - dj, jj - 1))
        out[g] = np.clip(np.where(leg[:, None], 2 * A - B, A + B - Cc), 0, 255)
    return out


def reduce(fine, F, texels_fine, reads=None):
    """uint8 [H', W', 3]: the level below `fine` [H, W, 3] (texels_fine > 2 a leg) of F faces.  reads: a list that takes
    (p [m], X [m, 4], Y [m, 4], w [m, 4]): coarse raster indices, the fine texels read for them and their bilinear weights (the
    texel beyond the hypotenuse's corner is read with the weight 0 at a point on the hypotenuse)."""
    Tf, Tc = int(texels_fine), (int(texels_fine) + 1) // 2
    assert Tf > 2
    lf, lc = T.layout(F, Tf), T.layout(F, Tc)
    W, H = lc[:2]
    p = np.arange(W * H, dtype=np.int64)
    f, i, j = T.owner(lc, p % W, p // W)
    out = np.zeros((W * H, 3), np.int64)
    k = np.nonzero(f < F)[0]
    if len(k):
        out[k] = _texel(np.asarray(fine, np.uint8), lf, Tf, Tc, f[k], i[k], j[k], reads, p[k])
    return out.astype(np.uint8).reshape(H, W, 3)


def pyramid(image, F, texels):
    """[(image_l, uv_l, T_l)] for every level; level 0 is `image` itself."""
    out = [(np.asarray(image, np.uint8), T.uvs(F, texels), int(texels))]
    for Tl in levels(texels)[1:]:
        out.append((reduce(out[-1][0], F, out[-1][2]), T.uvs(F, Tl), Tl))
    return out


def face_lod(verts, faces, view, near, texels, scale=1.0):
    """float32 [F]."""
    why, X, Y, _, _ = R.setup(verts, faces, view, near, False)
    Tl = levels(texels)
    L = len(Tl)
    S = np.abs(R.area2(X, Y))
    g = f32(scale) * (np.sqrt(S.astype(f32)) / f32(256))
    assert g.dtype == f32
    lod = np.full(len(why), f32(L - 1), f32)
    for l in range(L - 1):
        here = (g < f32(Tl[l] - 1)) & (g >= f32(Tl[l + 1] - 1))
        val = f32(l) + (f32(Tl[l] - 1) - g) / f32(Tl[l] - Tl[l + 1])
        assert val.dtype == f32
        lod = np.where(here, val, lod)
    lod = np.where((g >= f32(Tl[0] - 1)) | (L == 1) | (why != R.OK), f32(0), lod)
    return lod.astype(f32)


def sample(images, F, texels, face, bary, lod, per_face=False):
    """rgb float32 [n, 3]: images = the levels' [H_l, W_l, 3] arrays; lod [F] with per_face, else [n]."""
    Tl = levels(texels)
    L = len(Tl)
    assert len(images) == L
    face = np.asarray(face, np.int64)
    inside = (face >= 0) & (face < F)
    fz = np.where(inside, face, 0)
    wb, wc = T.clamp_bary(bary)
    lod = np.asarray(lod, f32)
    lam = lod[fz] if per_face else lod
    if not len(lam):
        return np.zeros((len(face), 3), f32)
    lam = np.where(lam > 0, lam, f32(0)).astype(f32)                     # NaN -> 0
    lam = np.where(lam < f32(L - 1), lam, f32(L - 1)).astype(f32)
    l = np.floor(lam).astype(np.int64)
    t = lam - l.astype(f32)
    out = np.zeros((len(face), 3), f32)
    for k in range(L):
        lay = T.layout(F, Tl[k])
        d = f32(Tl[k] - 1)
        a = np.nonzero(inside & (l == k))[0]
        if len(a):
            c0 = lookup(images[k], lay, fz[a], wb[a] * d, wc[a] * d)
            out[a] = c0
            b = a[t[a] != 0]
            if len(b):
                d1 = f32(Tl[k + 1] - 1)
                c1 = lookup(images[k + 1], T.layout(F, Tl[k + 1]), fz[b], wb[b] * d1, wc[b] * d1)
                tb = t[b][:, None]
                out[b] = ((f32(1) - tb) * out[b]) + (tb * c1)
    assert out.dtype == f32
    return out


def render(verts, faces, view, H, W, near, images, texels, background, scale=1.0, cull=False):
    """(rgb [H W, 3], face, bary, depth, acc, lod [F]): rasterise, lod per face, trilinear lookup, shade."""
    _, _, face, bary, depth, acc = R.render(verts, faces, view, H, W, near, cull)
    F = len(np.asarray(faces).reshape(-1, 3))
    lod = face_lod(verts, faces, view, near, texels, scale)
    looked = sample(images, F, texels, face, bary, lod, per_face=True)
    return R.shade(face, bary, faces, len(np.asarray(verts).reshape(-1, 3)), background, rgb_in=looked), face, bary, depth, acc, lod
