"""numpy reference of include/nerf_hip.h "morphological opening" (a helper module, not a conftest): the 6-neighbour erosion and
the geodesic reconstruction as shifted-slice ANDs / ORs of bool volumes, the value rule through a uint32 view as
tests/_ccl_ref.filter_volume, and the erode -> filter -> reconstruct pipeline on the reference's own components.  It calls
nothing of the code under test.  The constructed volumes the host and the GPU tests share live here too."""
import numpy as np

from tests import _ccl_ref as CC

MAX_RADIUS = 16                                                       # NERF_MORPH_MAX_RADIUS


def _shifted(a, axis, d):
    """a moved by d (+-1) along axis, False shifted in: out[.., n, ..] = a[.., n - d, ..] inside the lattice."""
    out = np.zeros_like(a)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if d > 0:
        src[axis], dst[axis] = slice(0, -1), slice(1, None)
    else:
        src[axis], dst[axis] = slice(1, None), slice(0, -1)
    out[tuple(dst)] = a[tuple(src)]
    return out


def erode_step(a):
    """a and its six neighbours; a neighbour beyond the lattice is outside."""
    out = a.copy()
    for axis in range(3):
        out &= _shifted(a, axis, 1) & _shifted(a, axis, -1)
    return out


def dilate_step(a):
    out = a.copy()
    for axis in range(3):
        out |= _shifted(a, axis, 1) | _shifted(a, axis, -1)
    return out


def erode_mask(m, radius):
    for _ in range(int(radius)):
        m = erode_step(m)
    return m


def reconstruct_mask(seeds, m, radius):
    """D_r of D_0 = seeds & m, D_{n+1} = dilate(D_n) & m: exactly `radius` steps."""
    d = seeds & m
    for _ in range(int(radius)):
        d = dilate_step(d) & m
    return d


def _drop(vol, iso, drop):
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    bits = vol.reshape(-1).view(np.uint32).copy()
    bits[np.asarray(drop).reshape(-1)] = np.array([iso], np.float32).view(np.uint32)[0]
    return bits.view(np.float32).reshape(vol.shape)


def erode(vol, iso, radius):
    """(core float32 [R, R, R], stats int64 [2] = (|M|, |E|))."""
    assert 1 <= int(radius) <= MAX_RADIUS
    m = CC.inside_mask(vol, iso)
    e = erode_mask(m, radius)
    return _drop(vol, iso, m & ~e), np.array([m.sum(), e.sum()], np.int64)


def reconstruct(vol, kept, iso, radius):
    """(out float32 [R, R, R], stats int64 [2] = (|K|, |D_r|))."""
    assert 1 <= int(radius) <= MAX_RADIUS
    m = CC.inside_mask(vol, iso)
    k = CC.inside_mask(kept, iso) & m
    d = reconstruct_mask(k, m, radius)
    return _drop(vol, iso, m & ~d), np.array([k.sum(), d.sum()], np.int64)


def open_components(vol, iso, radius, min_component=0, largest_only=False, comps=None):
    """erode -> (min_component > 1 or largest_only: CC.filter_volume of the core, on `comps` = the core's (labels, sizes, stats)
    when the caller has them) -> reconstruct."""
    kept, _ = erode(vol, iso, radius)
    if min_component > 1 or largest_only:
        kept = CC.filter_volume(kept, iso, min_component, largest_only, comps=comps)
    return reconstruct(vol, kept, iso, radius)[0]


# ------------------------------------------------------------------------------------------------ the direct definition
def erode_direct(m, radius):
    """p is in E exactly when every point within L1 distance r of p lies inside the lattice and in m (one shifted AND per offset
    of the ball: independent of erode_step's iteration)."""
    R = m.shape[0]
    r = int(radius)
    pad = np.zeros((R + 2 * r,) * 3, bool)
    pad[r:r + R, r:r + R, r:r + R] = m
    out = np.ones_like(m)
    for dz in range(-r, r + 1):
        for dy in range(-(r - abs(dz)), r - abs(dz) + 1):
            rest = r - abs(dz) - abs(dy)
            for dx in range(-rest, rest + 1):
                out &= pad[r + dz:r + dz + R, r + dy:r + dy + R, r + dx:r + dx + R]
    return out


def dilate_ball(a, radius):
    """a (+) ball_r inside the lattice (unconstrained dilation)."""
    for _ in range(int(radius)):
        a = dilate_step(a)
    return a


# ------------------------------------------------------------------------------------------------ marching cubes' edges
def crossing_edges(vol, iso):
    """(cross bool [R, R, R, 3], lower_inside bool [R, R, R, 3]) in marching cubes' vertex order when flattened (owner linear
    index, then axis x, y, z): the edge from q to q + e_a crosses; its owner q is the inside end."""
    ins = CC.inside_mask(vol, iso)
    R = ins.shape[0]
    cross = np.zeros((R, R, R, 3), bool)
    low = np.zeros((R, R, R, 3), bool)
    for a, axis in enumerate((2, 1, 0)):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, R - 1), slice(1, R)
        lo, hi = tuple(lo), tuple(hi)
        cross[lo + (a,)] = ins[lo] != ins[hi]
        low[lo + (a,)] = ins[lo]
    return cross, low


def original_edge_masks(vol, out, iso):
    """(in_out bool [V_out], in_vol bool [V_vol]): the vertices of marching cubes on `out` whose edge's outside end was outside in
    `vol` already, and the vertices of marching cubes on `vol` that those are, in order."""
    c0, _ = crossing_edges(vol, iso)
    c1, _ = crossing_edges(out, iso)
    both = c0 & c1                               # inside(out) is a subset of inside(vol): an edge crossing in both has the same ends
    return both.reshape(-1)[c1.reshape(-1)], both.reshape(-1)[c0.reshape(-1)]


# ------------------------------------------------------------------------------------------------ constructed volumes
def dumbbell(R=17, big=7, small=5, width=1, length=5, at=0, hi=2.0, x0=0):
    """(volume, bridge mask, big-cube mask): a big^3 cube at x = x0 and a small^3 cube joined along x by a `width` x `width` bar of
    `length` voxels; both cubes start at y = z = 1 and the bar runs at y = z = 1 + at.  at = 0 puts the bar on the cubes' edges:
    the voxels it touches have outside neighbours and erode, so the core is exactly the cubes' cores.  (A bar on the faces'
    centres, at = 2, makes the two face voxels it touches interior: they stay in the core at radius 1.)"""
    assert x0 + big + length + small <= R and 1 + big <= R and at + width <= small
    v = np.zeros((R, R, R), np.float32)
    v[1:1 + big, 1:1 + big, x0:x0 + big] = hi
    x1 = x0 + big + length
    v[1:1 + small, 1:1 + small, x1:x1 + small] = hi + 1.0
    bridge = np.zeros((R, R, R), bool)
    bridge[1 + at:1 + at + width, 1 + at:1 + at + width, x0 + big:x1] = True
    v[bridge] = hi + 0.5
    cube = np.zeros((R, R, R), bool)
    cube[1:1 + big, 1:1 + big, x0:x0 + big] = True
    return v, bridge, cube


def c_channel(R=17, gap=1):
    """(volume, seed mask, upper-arm mask) of a C: two arms (3 voxels thick) `gap` outside voxels apart along y, joined only by
    a spine at the far end in x.  The seeds are the lower arm up to 6 voxels short of the spine: gap + 1 from the upper arm in
    L1, more than 6 + gap + 1 steps from it inside the set."""
    v = np.zeros((R, R, R), np.float32)
    k0, k1 = R // 2 - 1, R // 2 + 2                                   # 3 thick in z
    j_lo = R // 2 - 3 - (gap - 1) // 2
    j_hi = j_lo + 3 + gap
    v[k0:k1, j_lo:j_lo + 3, 2:R - 2] = 2.0                            # lower arm
    v[k0:k1, j_hi:j_hi + 3, 2:R - 2] = 3.0                            # upper arm
    v[k0:k1, j_lo:j_hi + 3, R - 5:R - 2] = 2.5                        # spine
    lower = np.zeros((R, R, R), bool)
    lower[k0:k1, j_lo:j_lo + 3, 2:R - 11] = True
    upper = np.zeros((R, R, R), bool)
    upper[k0:k1, j_hi:j_hi + 3, 2:R - 2] = True
    return v, lower, upper


def smoothed_noise(R, seed, passes=2):
    """Gaussian noise box-blurred `passes` times along each axis (edge-padded): blobs a few voxels across, with thin necks."""
    v = np.random.default_rng(seed).standard_normal((R, R, R))
    for _ in range(passes):
        for axis in range(3):
            p = np.pad(v, [(1, 1) if a == axis else (0, 0) for a in range(3)], mode="edge")
            sl = lambda s: tuple(s if a == axis else slice(None) for a in range(3))
            v = (p[sl(slice(0, -2))] + p[sl(slice(1, -1))] + p[sl(slice(2, None))]) / 3.0
    return np.ascontiguousarray(v, dtype=np.float32)
