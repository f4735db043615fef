"""numpy reference of include/nerf_hip.h "mesh ray casting" (a helper module, not a test): the watertight face test in float64,
operator for operator (numpy rounds every operation on its own, as the library does with -ffp-contract=off; its float64 division
and the casts to float32 are correctly rounded); the brute force over every valid face with the lowest-index tie rule; the
stackless walk with its slab test and pruning rule, emulated ray by ray on tests/_bvh_ref.py's nodes and order, counting the faces
and the boxes it tests; and raycast_frame on top of either.  Validity of a face is tests/_distance_ref.py's."""
import functools

import numpy as np

from tests import _bvh_ref as B
from tests import _distance_ref as D

F32, F64 = np.float32, np.float64
STRIDE = 11
SLACK = 2.0 ** -30
NAN32 = B.NAN32
NONE = B.NONE


def pack(origins, dirs, tmin=0.0, tmax=np.inf):
    """float32 [n, 11]: o, d, tmin, tmax and three zeros."""
    o = np.asarray(origins, F32).reshape(-1, 3)
    rays = np.zeros((len(o), STRIDE), F32)
    rays[:, 0:3], rays[:, 3:6] = o, np.asarray(dirs, F32).reshape(-1, 3)
    rays[:, 6], rays[:, 7] = F32(tmin), F32(tmax)
    return rays


def valid_rays(rays):
    """bool [n]: o and d finite, d != 0, tmin and tmax not NaN, tmin >= 0."""
    r = np.asarray(rays, F32).reshape(-1, STRIDE)
    with np.errstate(invalid="ignore"):
        return (np.isfinite(r[:, :6]).all(1) & (r[:, 3:6] != 0).any(1) & ~np.isnan(r[:, 6]) & ~np.isnan(r[:, 7]) & (r[:, 6] >= 0))


class Frame:
    """The sheared frame of one valid ray: kx, ky, kz, Sx, Sy, Sz and the origin, all float64."""

    def __init__(self, row):
        row = np.asarray(row, F32)
        self.o, d = row[0:3].astype(F64), row[3:6].astype(F64)
        self.d = d
        self.tmin, self.tmax = row[6], row[7]
        kz, big = 0, abs(row[3])
        if abs(row[4]) > big:
            kz, big = 1, abs(row[4])
        if abs(row[5]) > big:
            kz = 2
        kx = (kz + 1) % 3
        ky = (kx + 1) % 3
        if d[kz] < 0.0:
            kx, ky = ky, kx
        self.kx, self.ky, self.kz = kx, ky, kz
        self.Sx, self.Sy, self.Sz = d[kx] / d[kz], d[ky] / d[kz], F64(1.0) / d[kz]
        with np.errstate(divide="ignore"):
            self.inv = np.where(d == 0.0, 0.0, F64(1.0) / np.where(d == 0.0, 1.0, d))

    def corner(self, p):
        """(x, y, z) float64 [...] of float32 corners p [..., 3]."""
        p = np.asarray(p, F32).astype(F64)
        ax, ay, az = p[..., self.kx] - self.o[self.kx], p[..., self.ky] - self.o[self.ky], p[..., self.kz] - self.o[self.kz]
        return ax - self.Sx * az, ay - self.Sy * az, self.Sz * az

    def faces(self, a, b, c):
        """(accepted bool, t float32, wb float32, wc float32) of the triangles (a, b, c) [m, 3]: the header's face test."""
        with np.errstate(all="ignore"):
            Ax, Ay, Az = self.corner(a)
            Bx, By, Bz = self.corner(b)
            Cx, Cy, Cz = self.corner(c)
            U = Cx * By - Cy * Bx
            V = Ax * Cy - Ay * Cx
            W = Bx * Ay - By * Ax
            mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
            det = (U + V) + W
            t64 = ((U * Az + V * Bz) + W * Cz) / det
            t = t64.astype(F32) + F32(0.0)
            ok = ~mixed & (det != 0.0) & (self.tmin <= t) & (t <= self.tmax)
            return ok, t, (V / det).astype(F32), (W / det).astype(F32)

    def box(self, node, eta):
        """(met, enter, exit) of a node's six floats widened by eta: the slab test."""
        if node[0] > node[3]:
            return False, 0.0, 0.0
        lo, hi = node[:3].astype(F64) - eta, node[3:].astype(F64) + eta
        en, ex, inside = -np.inf, np.inf, True
        for a in range(3):
            if self.inv[a] == 0.0:
                inside = inside and bool(self.o[a] >= lo[a]) and bool(self.o[a] <= hi[a])
            else:
                t0, t1 = (lo[a] - self.o[a]) * self.inv[a], (hi[a] - self.o[a]) * self.inv[a]
                if self.inv[a] < 0.0:
                    t0, t1 = t1, t0
                en, ex = max(en, t0), min(ex, t1)
        return bool(inside and en <= ex), en, ex

    def skip(self, met, en, ex, best):
        if not met:
            return True
        with np.errstate(over="ignore"):
            en32, ex32 = F32(en), F32(ex)
        tbest = np.array([best >> 32], np.uint32).view(F32)[0]
        return bool(ex32 < self.tmin or en32 > self.tmax or en32 > tbest)


def _key(t, f):
    return (int(np.array([t], F32).view(np.uint32)[0]) << 32) | int(f)


def brute_force(rays, verts, faces):
    """(t [n] float32, face [n] int32, bary [n, 2] float32): the smallest key (bits of t) 2^32 + f over the accepted hits of every
    valid face; (+inf, -1, NaN, NaN) for a miss and (NaN, -1, NaN, NaN) for a ray without an answer."""
    rays = np.asarray(rays, F32).reshape(-1, STRIDE)
    ok, a, b, c, _ = D.corners(verts, faces)
    idx = np.nonzero(ok)[0]
    a, b, c = a[ok], b[ok], c[ok]
    n = len(rays)
    t, face, bary = np.full(n, np.inf, F32), np.full(n, -1, np.int32), np.full((n, 2), NAN32, F32)
    good = valid_rays(rays)
    t[~good] = NAN32
    if not len(idx):
        return t, face, bary
    for i in np.nonzero(good)[0]:
        hit, ti, wb, wc = Frame(rays[i]).faces(a, b, c)
        if not hit.any():
            continue
        keys = (ti.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
        j = int(np.argmin(np.where(hit, keys, np.uint64(NONE))))
        t[i], face[i], bary[i] = ti[j], idx[j], (wb[j], wc[j])
    return t, face, bary


class Caster:
    """The hierarchy of one mesh (tests/_bvh_ref.py's Tree) and the kernel's walk on it, step for step."""

    def __init__(self, verts, faces, lo=D.LO, hi=D.HI):
        self.tree = B.Tree(verts, faces, lo, hi)

    def one(self, row, any_hit=False):
        """(key of the answer, faces tested, boxes tested) for one valid ray."""
        tr = self.tree
        fr = Frame(row)
        root = tr.nodes[1]
        o32 = np.asarray(row, F32)[0:3]
        S = F32(max(np.abs(o32).max(), np.abs(root).max(), tr.box_abs)) if root[0] <= root[3] else F32(max(np.abs(o32).max(), tr.box_abs))
        eta = float(S) * SLACK
        best, tested, boxes = NONE, 0, 1
        if fr.skip(*fr.box(root, eta), best):
            return best, tested, boxes
        node, trail, P = 1, 0, tr.P
        while True:
            up = False
            if node >= P:
                s0 = B.LEAF * (node - P)
                for s in range(s0, min(s0 + B.LEAF, tr.F)):
                    f = int(tr.order[s])
                    if f < 0:
                        continue
                    if any_hit and best != NONE:
                        break
                    tested += 1
                    hit, t, _, _ = fr.faces(tr.a[f][None], tr.b[f][None], tr.c[f][None])
                    if hit[0]:
                        best = min(best, _key(t[0], f))
                if any_hit and best != NONE:
                    return best, tested, boxes
                up = True
            else:
                ml, el, xl = fr.box(tr.nodes[2 * node], eta)
                mr, er, xr = fr.box(tr.nodes[2 * node + 1], eta)
                boxes += 2
                left_ok, right_ok = not fr.skip(ml, el, xl, best), not fr.skip(mr, er, xr, best)
                right = (er < el) if (left_ok and right_ok) else right_ok
                near_ok, far_ok = (right_ok, left_ok) if right else (left_ok, right_ok)
                if near_ok:
                    node, trail = 2 * node + int(right), ((trail << 1) | int(far_ok)) & 0xFFFFFFFF
                else:
                    up = True
            if not up:
                continue
            while True:
                if trail == 0:
                    return best, tested, boxes
                k = (trail & -trail).bit_length() - 1
                trail = (trail >> k) & ~1
                node = (node >> k) ^ 1
                boxes += 1
                if not fr.skip(*fr.box(tr.nodes[node], eta), best):
                    break

    def cast(self, rays):
        """(t [n] float32, face [n] int32, bary [n, 2] float32, visits [n, 2] int32)."""
        rays = np.asarray(rays, F32).reshape(-1, STRIDE)
        n, tr = len(rays), self.tree
        bits, face = np.full(n, D.NAN_BITS, np.uint32), np.full(n, -1, np.int32)
        bary, visits = np.full((n, 2), NAN32, F32), np.zeros((n, 2), np.int32)
        for i in np.nonzero(valid_rays(rays))[0]:
            best, visits[i, 0], visits[i, 1] = self.one(rays[i])
            bits[i] = best >> 32
            f = face[i] = np.array([best & 0xFFFFFFFF], np.uint32).view(np.int32)[0]
            if f >= 0:
                _, _, wb, wc = Frame(rays[i]).faces(tr.a[f][None], tr.b[f][None], tr.c[f][None])
                bary[i] = wb[0], wc[0]
        return bits.view(F32), face, bary, visits

    def any(self, rays):
        """uint8 [n]: 1 where the walk, left at the first accepted hit, found one."""
        rays = np.asarray(rays, F32).reshape(-1, STRIDE)
        hit = np.zeros(len(rays), np.uint8)
        for i in np.nonzero(valid_rays(rays))[0]:
            hit[i] = self.one(rays[i], any_hit=True)[0] != NONE
        return hit


def frame_of(t, face, bary, H, W):
    """(face [H, W], bary [H, W, 2], depth [H, W], acc [H, W]) from a cast in pixel order: depth = t where hit, else 0; bary 0 at a miss."""
    hit = face >= 0
    depth = np.where(hit, t, F32(0.0)).astype(F32)
    return (face.reshape(H, W), np.where(hit[:, None], bary, F32(0.0)).astype(F32).reshape(H, W, 2), depth.reshape(H, W),
            hit.astype(F32).reshape(H, W))


def bounds(verts):
    """(lo [3], hi [3]) as engine.mesh.raycast._mesh_bounds picks them for raycast_frame: about the finite vertices, padded."""
    v = np.asarray(verts, F32).reshape(-1, 3)
    v = v[np.isfinite(v).all(1)]
    if not len(v):
        return [-1.0] * 3, [1.0] * 3
    mn, mx = v.min(0).astype(F64), v.max(0).astype(F64)
    pad = max(1e-6, 1e-3 * float((mx - mn).max()), 1e-6 * float(max(np.abs(mn).max(), np.abs(mx).max())))
    return [float(x) - pad for x in mn], [float(x) + pad for x in mx]


@functools.lru_cache(maxsize=None)
def sphere24_frame(H=64, W=64, near=0.01):
    """(verts, faces, c2w, K, the mirror's raycast_frame + visits) of sphere24 from the first pose of the rasteriser's tests:
    computed once, shared by the host and the GPU tests, read-only."""
    from tests import _raster_ref as R
    from tests import _ray_ref as RR
    from tests import _smooth_ref as S
    v, f = D.MESHES["sphere24"]()
    c2w, K = R.look_at(S.CENTRE + [2.6, 1.1, 2.2], S.CENTRE), R.intrinsics(H, W)
    rays = RR.ray_gen(np.arange(H * W), W, K, c2w, near, np.inf)[0]
    t, face, bary, visits = Caster(v, f, *bounds(v)).cast(rays)
    out = frame_of(t, face, bary, H, W) + (visits.reshape(H, W, 2),)
    for a in out:
        a.setflags(write=False)
    return v, f, c2w, K, out


# ------------------------------------------------------------------------------------------------ the shared ray sets
def between(points, n, seed=11):
    """n rays between seeded pairs of finite `points`: d = target - origin in float32, tmin 0, tmax +inf."""
    p = np.asarray(points, F32)
    p = p[np.isfinite(p).all(1)]
    rng = np.random.default_rng(seed)
    i, j = rng.integers(0, len(p), n), rng.integers(0, len(p), n)
    return pack(p[i], p[j] - p[i])


def far_rays(lo=D.LO, hi=D.HI):
    """From B.far_points() towards the centre of the box and away from it."""
    p = B.far_points(lo, hi)
    ctr = ((np.array(lo) + np.array(hi)) / 2).astype(F32)
    return np.concatenate([pack(p, ctr - p), pack(p, p - ctr)])


def cube_plane_rays():
    """Axis-parallel rays lying exactly in the planes of the faces of D.cube(): d_a = 0 with o_a on min_a or max_a, for every axis
    pair, from outside the cube and from a point of its edge."""
    v, _ = D.cube()
    mn, mx = v.min(0), v.max(0)
    o, d = [], []
    for a in range(3):                                                 # the axis whose slab the ray lies on
        for side in (mn, mx):
            for b in range(3):                                         # the axis it runs along
                if b == a:
                    continue
                c = 3 - a - b
                for start in (mn[b] - 1.0, mn[b]):
                    for oc in (mn[c] + 0.25, mn[c]):
                        p = np.zeros(3)
                        p[a], p[b], p[c] = side[a], start, oc
                        e = np.zeros(3)
                        e[b] = 1.0
                        o.append(p)
                        d.append(e)
                        o.append(p + e * (mx[b] - mn[b] + 2.0))
                        d.append(-e)
    return pack(np.array(o), np.array(d))


def surface_rays(verts, faces, n=24, seed=13):
    """Rays that start on the surface: at corners and edge midpoints of valid faces, towards seeded directions."""
    ok, a, b, c, _ = D.corners(verts, faces)
    if not ok.any():
        return pack(np.zeros((0, 3)), np.zeros((0, 3)))
    rng = np.random.default_rng(seed)
    k = rng.integers(0, int(ok.sum()), n)
    start = np.where((np.arange(n) % 2 == 0)[:, None], a[ok][k], (a[ok][k] + b[ok][k]) * F32(0.5))
    return pack(start, rng.standard_normal((n, 3)))


def bad_rays():
    """Rays without an answer: zero and non-finite d, a non-finite o, NaN tmin and tmax, a negative tmin."""
    r = pack(np.tile([0.0, 0.75, 1.5], (7, 1)), np.tile([1.0, 0.0, 0.0], (7, 1)))
    r[0, 3:6] = 0.0
    r[1, 4] = np.inf
    r[2, 5] = np.nan
    r[3, 0] = np.inf
    r[4, 6] = np.nan
    r[5, 7] = np.nan
    r[6, 6] = -1.0
    return r


def ray_set(verts, faces, n=300):
    """The rays every mesh is cast with: n between query points, the far ones, the cube's plane rays, rays from the surface, the
    bad ones and one with tmin > tmax."""
    v = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    pts = D.query_points(v, f, 300, 5) if len(v) else D.query_points(*D.cube(), 300, 5)
    back = pack([[0.0, 0.75, 1.5]], [[1.0, 0.25, 0.125]], 2.0, 1.0)
    return np.concatenate([between(pts, n), far_rays(), cube_plane_rays(), surface_rays(v, f), bad_rays(), back])


MESHES = dict(D.MESHES)
MESHES.update({f"small{F}": functools.partial(B.small, F) for F in (0, 1, 3, 4, 5, 8, 9, 17)})
MESHES.update({"all_invalid": B.all_invalid, "doubled": B.doubled, "cube": D.cube})


@functools.lru_cache(maxsize=None)
def case(name):
    """(verts, faces, rays, (t, face, bary) of the brute force, (t, face, bary, visits) of the walk, any-hit of the walk):
    computed once, shared by the host and the GPU tests, read-only."""
    v, f = MESHES[name]()
    v, f = np.asarray(v, F32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3)
    rays = ray_set(v, f)
    brute = brute_force(rays, v, f)
    caster = Caster(v, f)
    walk, hit = caster.cast(rays), caster.any(rays)
    for a in (v, f, rays, hit) + brute + walk:
        a.setflags(write=False)
    return v, f, rays, brute, walk, hit
