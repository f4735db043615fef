"""numpy float32 emulation of include/nerf_hip.h "TSDF fusion" (csrc/tsdf.hip): every intermediate is an np.float32 array, one
rounding per operation, in the header's order (numpy's float32 +, -, *, / are IEEE, correctly rounded), a plain loop over the
views; the camera is tests/_camera_ref.py's.  Also the analytic depth / opacity maps of a sphere for a pinhole camera of the project's convention (camera directions
[(col - cx) / fx, -(row - cy) / fy, -1], c2w [3, 4])."""
import numpy as np

from tests import _mesh_ref as M
from tests._camera_ref import intrinsics, look_at, nearest, project, view_of as view_floats  # noqa: F401  (the tests' names)

_F = np.float32
MAX_VIEWS = 16


class State:
    """D, Wt float32 [R^3] and flags uint8 [R^3] in linear order i + R (j + R k)."""

    def __init__(self, R):
        self.R = int(R)
        self.D = np.zeros(self.R ** 3, _F)
        self.Wt = np.zeros(self.R ** 3, _F)
        self.flags = np.zeros(self.R ** 3, np.uint8)

    def copy(self):
        s = State(self.R)
        s.D, s.Wt, s.flags = self.D.copy(), self.Wt.copy(), self.flags.copy()
        return s


def classify_view(R, lo, hi, view, H, W, depth, acc, tau, acc_min, far, carve):
    """The per-voxel rule of one view as masks over the R^3 voxels, each voxel in exactly one of
    behind (!(zc > 0)), outside (off the image or not finite), nan_acc, nan_depth (acc fine, depth NaN), low_skipped (acc < acc_min,
    not carved), empty (acc < acc_min, carved: d = 1), occluded (e < -tau), nan_e, surface (d = min(1, e / tau));
    plus "d" (float32, valid where empty | surface), "zero_pixel" (acc == 0 and depth == 0 under the voxel) and "zc"."""
    with np.errstate(all="ignore"):
        p = M.lattice_points(R, lo, hi)                                    # [R^3, 3] float32
        tau, acc_min, far = _F(tau), _F(acc_min), _F(far)
        depth = np.asarray(depth, _F).reshape(-1)
        acc = np.asarray(acc, _F).reshape(-1)
        assert depth.size == H * W and acc.size == H * W
        u, v, zc = project(p, view)
        front = zc > 0
        in_map, pix = nearest(u, v, H, W)                                  # NaN and +-inf fail
        inside = front & in_map
        a, s = acc[pix], depth[pix]
        nan_acc = inside & np.isnan(a)
        nan_depth = inside & ~np.isnan(a) & np.isnan(s)
        ok = inside & ~np.isnan(a) & ~np.isnan(s)
        low = ok & (a < acc_min)
        empty = low & bool(carve) & (zc <= far)
        e = ((s / a).astype(_F) - zc).astype(_F)
        neg_tau = (_F(0.0) - tau).astype(_F)
        occluded = ok & ~low & (e < neg_tau)
        surface = ok & ~low & (e >= neg_tau)
        nan_e = ok & ~low & ~occluded & ~surface
        d = np.where(empty, _F(1.0), np.minimum(_F(1.0), (e / tau).astype(_F))).astype(_F)
    return {"behind": ~front, "outside": front & ~inside, "nan_acc": nan_acc, "nan_depth": nan_depth, "low_skipped": low & ~empty,
            "empty": empty, "occluded": occluded, "nan_e": nan_e, "surface": surface, "d": d,
            "zero_pixel": ok & (a == 0) & (s == 0), "zc": zc}


BRANCHES = ("behind", "outside", "nan_acc", "nan_depth", "low_skipped", "empty", "occluded", "nan_e", "surface")


def integrate_view(st, lo, hi, view, H, W, depth, acc, tau, acc_min, far, carve):
    """One view folded into `st` in place.  view: 16 float32 (view_floats); depth, acc: float32 [H W]."""
    c = classify_view(st.R, lo, hi, view, H, W, depth, acc, tau, acc_min, far, carve)
    assert sum(c[k].astype(np.int64) for k in BRANCHES).min() == 1 == sum(c[k].astype(np.int64) for k in BRANCHES).max()
    with np.errstate(all="ignore"):
        obs = c["surface"] | c["empty"]
        Wn = (st.Wt + _F(1.0)).astype(_F)
        Dn = (((st.D * st.Wt).astype(_F) + c["d"]).astype(_F) / Wn).astype(_F)
        st.D = np.where(obs, Dn, st.D).astype(_F)
        st.Wt = np.where(obs, Wn, st.Wt).astype(_F)
        st.flags = np.where(c["occluded"], st.flags | 1, st.flags).astype(np.uint8)
    return st


def integrate(st, lo, hi, views, H, W, depth, acc, tau, acc_min, far, carve):
    """views [n, 16], depth / acc [n, H W], folded in order."""
    views = np.asarray(views, _F).reshape(-1, 16)
    depth = np.asarray(depth, _F).reshape(len(views), -1)
    acc = np.asarray(acc, _F).reshape(len(views), -1)
    for s in range(len(views)):
        integrate_view(st, lo, hi, views[s], H, W, depth[s], acc[s], tau, acc_min, far, carve)
    return st


def volume(st, min_views=1):
    """float32 [R, R, R]: 0 - D where Wt >= min_views, else +1 where flag bit 0 is set, else -1."""
    assert min_views >= 1
    seen = st.Wt >= _F(min_views)
    v = np.where(seen, (_F(0.0) - st.D).astype(_F), np.where(st.flags & 1, _F(1.0), _F(-1.0))).astype(_F)
    return v.reshape(st.R, st.R, st.R)


def default_trunc(R, lo, hi):
    """4 max(h_a) as a float32 (engine.mesh.TSDFVolume's trunc=None)."""
    return float(_F(4.0) * M.spacing(R, lo, hi).max())


# ------------------------------------------------------------------------------------------------ analytic fixtures
def sphere_maps(c2w, K, H, W, radius, centre=(0.0, 0.0, 0.0)):
    """(depth [H W], acc [H W]) float32 of an opaque sphere: acc = 1 and depth = the ray parameter z of the first hit of
    o + z d, d = R [(col - cx) / fx, -(row - cy) / fy, -1] (distance along the optical axis); both 0 where the ray misses."""
    c2w, K = np.asarray(c2w, np.float64), np.asarray(K, np.float64)
    col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dc = np.stack([(col - K[0, 2]) / K[0, 0], -(row - K[1, 2]) / K[1, 1], -np.ones_like(col)], -1).reshape(-1, 3)
    d = dc @ c2w[:3, :3].T
    oc = c2w[:3, 3] - np.asarray(centre, np.float64)
    A = (d * d).sum(-1)
    B = 2.0 * (d @ oc)
    Cc = oc @ oc - radius * radius
    disc = B * B - 4 * A * Cc
    hit = disc > 0
    z = np.where(hit, (-B - np.sqrt(np.where(hit, disc, 0.0))) / (2 * A), 0.0)
    hit &= z > 0
    return np.where(hit, z, 0.0).astype(_F), hit.astype(_F)


def six_cameras(dist=3.0):
    """c2w of 6 cameras on the +-x, +-y, +-z axes at `dist`, looking at the origin."""
    eyes = [(dist, 0, 0), (-dist, 0, 0), (0, dist, 0), (0, -dist, 0), (0, 0, dist), (0, 0, -dist)]
    return [look_at(e) for e in eyes]


def sphere_fixture(R=32, bound=1.0, radius=0.6, H=96, W=96, dist=3.0):
    """The 6-view sphere: (State after fusion, lo, hi, tau, views [6, 16], depth [6, H W], acc [6, H W], H, W)."""
    lo, hi = [-bound] * 3, [bound] * 3
    K = intrinsics(H, W, fov=0.9)
    cams = six_cameras(dist)
    views = np.stack([view_floats(c, K) for c in cams])
    maps = [sphere_maps(c, K, H, W, radius) for c in cams]
    depth = np.stack([m[0] for m in maps])
    acc = np.stack([m[1] for m in maps])
    tau = default_trunc(R, lo, hi)
    st = integrate(State(R), lo, hi, views, H, W, depth, acc, tau, 0.5, 6.0, True)
    return st, lo, hi, tau, views, depth, acc, H, W
