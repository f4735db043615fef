"""numpy reference of include/nerf_hip.h "view-projected texture" (a helper module, not a test): the texels are those of
tests/_texture_ref.py, the camera that of tests/_camera_ref.py, every float step a float32 array operation in the header's order
(numpy rounds each on its own; its division and square root are correctly rounded).  Same state, image and seen as
csrc/project.hip, bit for bit."""
import numpy as np

from tests import _camera_ref as C
from tests import _raster_ref as R
from tests import _texture_ref as TX

F32 = np.float32
BLEND, BEST = 0, 1
MODES = {"blend": BLEND, "best": BEST}
MAX_VIEWS = 16


def texels(verts, normals, faces, T):
    """(ok [P] bool, x [P, 3], n [P, 3] float32) of all texels of the atlas in raster order: position and unit normal of
    nerf_texture_rows (row[0:3] = x, row[3:6] = -n); ok is False for a texel of no face or of a face with a bad index."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    lay = TX.layout(len(faces), T)
    W, H = lay[:2]
    p = np.arange(W * H, dtype=np.int64)
    f = TX.owner(lay, p % W, p // W)[0]
    ok, _ = TX._good(faces, np.where(f < len(faces), f, -1), len(np.asarray(verts).reshape(-1, 3)))
    rows = TX.texel_rows(verts, normals, faces, T)
    return ok, rows[:, 0:3].copy(), (-rows[:, 3:6]).astype(F32)


def observe(view, image, depth, acc, x, n, near, depth_tol, cos_min, acc_min):
    """(got [P] bool, w [P], c [P, 3] float32): what one view says about the points x with the normals n.  view float32 [16],
    image [H, W, 3], depth and acc [H W] or [H, W]."""
    image = np.asarray(image, F32)
    H, W = image.shape[:2]
    depth, acc = np.asarray(depth, F32).reshape(-1), np.asarray(acc, F32).reshape(-1)
    x, n = np.asarray(x, F32).reshape(-1, 3), np.asarray(n, F32).reshape(-1, 3)
    t = np.asarray(view, F32)[[3, 7, 11]]
    fW, fH = F32(W), F32(H)
    with np.errstate(all="ignore"):
        u, v, zc = C.project(x, view)
        got = zc >= F32(near)
        e = t[None, :] - x
        L = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        cosv = ((n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]) / L
        got &= cosv >= F32(cos_min)
        inside, pix = C.nearest(u, v, H, W)
        got &= inside
        a, s = acc[pix], depth[pix]
        got &= ~(np.isnan(a) | np.isnan(s) | (a < F32(acc_min)))
        ez = s / a - zc
        got &= ez >= F32(0.0) - F32(depth_tol)
        x0, y0 = np.floor(u), np.floor(v)
        room = (x0 >= 0) & (x0 + F32(1) <= fW - F32(1)) & (y0 >= 0) & (y0 + F32(1) <= fH - F32(1))
        got &= room
        fx, fy = u - x0, v - y0
        gx, gy = F32(1) - fx, F32(1) - fy
        w00, w10, w01, w11 = (gx * gy)[:, None], (fx * gy)[:, None], (gx * fy)[:, None], (fx * fy)[:, None]
        ix, iy = np.where(room, x0, 0).astype(np.int64), np.where(room, y0, 0).astype(np.int64)
        ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)           # (only where there is no room)
        c = ((w00 * image[iy, ix] + w10 * image[iy, ix1]) + w01 * image[iy1, ix]) + w11 * image[iy1, ix1]
        got &= ~np.isnan(c).any(1)
    assert u.dtype == F32 and cosv.dtype == F32 and ez.dtype == F32 and c.dtype == F32
    return got, cosv.astype(F32), c.astype(F32)


def fold(state, got, w, c, mode):
    """One view's observations into state [P, 4], in place."""
    with np.errstate(all="ignore"):
        if mode == BLEND:
            new = np.concatenate([state[:, :3] + w[:, None] * c, (state[:, 3] + w)[:, None]], 1)
            take = got
        else:
            new = np.concatenate([c, w[:, None]], 1)
            take = got & (w > state[:, 3])
    assert new.dtype == F32
    state[take] = new[take]
    return state


def accumulate(state, verts, normals, faces, T, views, images, depth, acc, near, depth_tol, cos_min, acc_min, mode):
    """nerf_project_accumulate over the whole atlas, view after view, in place.  views [n, 16], images [n, H, W, 3], depth and
    acc [n, H W]; any n (a launch of the library takes at most MAX_VIEWS, and a split changes nothing)."""
    ok, x, n = texels(verts, normals, faces, T)
    for k in range(len(views)):
        got, w, c = observe(views[k], images[k], depth[k], acc[k], x, n, near, depth_tol, cos_min, acc_min)
        fold(state, got & ok, w, c, mode)
    return state


def finish(state, lay, mode, fallback=None):
    """(image uint8 [H, W, 3], seen uint8 [H, W]) of state [P, 4]."""
    W, H = lay[:2]
    state = np.asarray(state, F32).reshape(W * H, 4)
    with np.errstate(all="ignore"):
        got = state[:, 3] > 0
        c = state[:, :3] / state[:, 3:4] if mode == BLEND else state[:, :3]
        b = np.rint(F32(255) * TX._unit(c)).astype(np.uint8)
    assert c.dtype == F32
    other = np.zeros((W * H, 3), np.uint8) if fallback is None else np.asarray(fallback, np.uint8).reshape(W * H, 3)
    return np.where(got[:, None], b, other).astype(np.uint8).reshape(H, W, 3), got.astype(np.uint8).reshape(H, W)


def maps(verts, faces, view, H, W, near):
    """(depth, acc) [H W] float32 of the mesh from the view: tests/_raster_ref.py's render."""
    out = R.render(verts, faces, view, H, W, near)
    return out[4], out[5]


def bake(verts, normals, faces, T, views, images, near, depth_tol, cos_min, acc_min=0.5, mode=BLEND, fallback=None, depth=None, acc=None):
    """(image, seen, state) of engine.mesh.project_texture: the maps are the reference rasteriser's unless given."""
    faces_ = np.asarray(faces, np.int64).reshape(-1, 3)
    lay = TX.layout(len(faces_), T)
    images = np.asarray(images, F32)
    H, W = images.shape[1:3]
    if depth is None:
        both = [maps(verts, faces, v, H, W, near) for v in views]
        depth, acc = np.stack([m[0] for m in both]), np.stack([m[1] for m in both])
    state = np.zeros((lay[0] * lay[1], 4), F32)
    accumulate(state, verts, normals, faces, T, views, images, depth, acc, near, depth_tol, cos_min, acc_min, mode)
    image, seen = finish(state, lay, mode, fallback)
    return image, seen, state
