"""Host reference of the hash-grid kernels (a helper module for the tests, not a conftest; csrc/encode.hip, csrc/adam.hip are the
product).

Everything is numpy float32 with ONE rounding per operation, in the operation order of csrc/hash_common.h / encode.hip / adam.hip
(the library is built with -ffp-contract=off and keeps f32 subnormals), so the kernels are held to it bit for bit:
  points     ((o + z d) * scale) + offset per axis                                               (hash_common.h: point_of)
  corners    xs = p * float32(N_l), off = xs - floor(xs), corner ids uint32(int32(floor / ceil)), hashed with uint32 wrap-around
  encode     the nested lerps of trilerp                                                          (hash_common.h: trilerp)
  sh         the real SH basis of sh_eval                                                         (hash_common.h: sh_eval)
  addends    g * w_z * w_y * w_x, left to right                                                   (encode.hip: hashgrid_bwd_kernel)
  to_fixed   2^-52 fixed point, saturation / poison codes                                         (hash_common.h: nerf_to_fixed)
  scatter    the exact int64 sum per entry (mod 2^64), or the float64 sum with sum |a| and the addend count
  adam_ex    nerf_adam_step(_ex / _shadow)                                                        (adam.hip: adam_kernel)
"""
import ctypes
import ctypes.util

import numpy as np

f32 = np.float32
ONE = f32(1.0)
P1 = np.uint32(2654435761)
P2 = np.uint32(805459861)
FIX_SHIFT = 52
FIX_SATURATED = (1 << 60) + (1 << 59)
FIX_POISON = 1 << 61
HC_CAP, HC_PROBES = 1024, 32          # the LDS write-combining table of hashgrid_bwd_combine_kernel


def points(rays, z, n, scale=1.0, offset=0.0):
    """[M, 3] float32 sample positions of rays [B, 11] and depths z [B n] (row m belongs to ray m // n)."""
    rays = np.asarray(rays, dtype=f32)
    z = np.asarray(z, dtype=f32).reshape(-1)
    r = rays[np.arange(z.shape[0]) // n]
    return (r[:, 0:3] + z[:, None] * r[:, 3:6]) * f32(scale) + f32(offset)


def hash3(cx, cy, cz, T):
    return (cx ^ (cy * P1) ^ (cz * P2)) & np.uint32(T - 1)


def _cells(p, res):
    """xs = p * N_l; floor, ceil (as uint32 corner ids), offset = xs - floor."""
    xs = np.asarray(p, dtype=f32) * f32(res)
    fl, ce = np.floor(xs), np.ceil(xs)
    with np.errstate(invalid="ignore"):        # NaN positions: any id (their features are NaN whatever they gather)
        cf = np.where(np.isfinite(fl), fl, 0).astype(np.int32).view(np.uint32)
        cc = np.where(np.isfinite(ce), ce, 0).astype(np.int32).view(np.uint32)
    return cf, cc, xs - fl


# hash_common.h:93: 0=(c,c,c) 1=(c,f,c) 2=(f,f,c) 3=(f,c,c) 4=(c,c,f) 5=(c,f,f) 6=(f,f,f) 7=(f,c,f); 1 = ceil per axis (x, y, z)
CORNERS = ((1, 1, 1), (1, 0, 1), (0, 0, 1), (0, 1, 1), (1, 1, 0), (1, 0, 0), (0, 0, 0), (0, 1, 0))


def corners(p, res, T):
    """uint32 [M, 8] table rows of the 8 corners (numbering above), float32 [M, 3] offsets."""
    cf, cc, off = _cells(p, res)
    idx = np.stack([hash3(*[(cc if c else cf)[:, a] for a, c in enumerate(k)], T) for k in CORNERS], 1)
    return idx, off


def encode(p, tables, res):
    """[M, L F] hash features of positions p [M, 3]; tables [L, T, F] float32."""
    tables = np.asarray(tables, dtype=f32)
    L, T, F = tables.shape
    out = np.empty((p.shape[0], L * F), dtype=f32)
    for l in range(L):
        idx, off = corners(p, res[l], T)
        e = tables[l][idx]                                   # [M, 8, F]
        ox, oy, oz = off[:, 0:1], off[:, 1:2], off[:, 2:3]
        h03 = e[:, 0] * ox + e[:, 3] * (ONE - ox)
        h12 = e[:, 1] * ox + e[:, 2] * (ONE - ox)
        h56 = e[:, 5] * ox + e[:, 6] * (ONE - ox)
        h47 = e[:, 4] * ox + e[:, 7] * (ONE - ox)
        h0312 = h03 * oy + h12 * (ONE - oy)
        h4756 = h47 * oy + h56 * (ONE - oy)
        out[:, l * F:(l + 1) * F] = h0312 * oz + h4756 * (ONE - oz)
    return out


def sh(dirs, deg):
    """[M, (deg+1)^2] real SH basis, sh_eval's operation order (C++ float literals and integer factors as float32)."""
    d = np.asarray(dirs, dtype=f32)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c = lambda v: f32(v)                                     # noqa: E731
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    o = [np.full_like(x, c(0.28209479177387814))]
    if deg >= 1:
        o += [c(0.4886025119029199) * y, c(0.4886025119029199) * z, c(0.4886025119029199) * x]
    if deg >= 2:
        o += [c(1.0925484305920792) * xy, c(1.0925484305920792) * yz, c(0.9461746957575601) * zz - c(0.31539156525251999),
              c(1.0925484305920792) * xz, c(0.5462742152960396) * (xx - yy)]
    if deg >= 3:
        o += [c(0.5900435899266435) * y * (c(3) * xx - yy), c(2.890611442640554) * xy * z,
              c(0.4570457994644658) * y * (c(5) * zz - c(1)), c(0.3731763325901154) * z * (c(5) * zz - c(3)),
              c(0.4570457994644658) * x * (c(5) * zz - c(1)), c(1.445305721320277) * z * (xx - yy),
              c(0.5900435899266435) * x * (xx - c(3) * yy)]
    if deg >= 4:
        o += [c(2.5033429417967046) * xy * (xx - yy), c(1.7701307697799304) * yz * (c(3) * xx - yy),
              c(0.9461746957575601) * xy * (c(7) * zz - c(1)), c(0.6690465435572892) * yz * (c(7) * zz - c(3)),
              c(0.10578554691520431) * (c(35) * zz * zz - c(30) * zz + c(3)),
              c(0.6690465435572892) * xz * (c(7) * zz - c(3)), c(0.47308734787878004) * (xx - yy) * (c(7) * zz - c(1)),
              c(1.7701307697799304) * xz * (xx - c(3) * yy),
              c(0.6258357354491761) * (xx * (xx - c(3) * yy) - yy * (c(3) * xx - yy))]
    return np.stack(o, 1).astype(f32)


def addends(p, d_out, res, T, F, L, levels=None):
    """Every addend of the table-gradient scatter: (int64 flat index into [L, T, F], float32 value) for each (sample, level in
    `levels`, feature, corner).  d_out [M, L F] is the upstream gradient of all L levels."""
    d_out = np.asarray(d_out, dtype=f32).reshape(p.shape[0], L, F)
    idxs, vals = [], []
    for l in (range(L) if levels is None else levels):
        cf, cc, off = _cells(p, res[l])
        w = ((ONE - off), off)                               # weight of the floor (0) / ceil (1) side, per axis
        for k in CORNERS:
            h = hash3(*[(cc if c else cf)[:, a] for a, c in enumerate(k)], T).astype(np.int64)
            wx, wy, wz = w[k[0]][:, 0:1], w[k[1]][:, 1:2], w[k[2]][:, 2:3]
            idxs.append((l * T + h)[:, None] * F + np.arange(F, dtype=np.int64)[None, :])
            with np.errstate(invalid="ignore", over="ignore"):        # NaN / Inf upstream gradients stay NaN / Inf
                vals.append(d_out[:, l, :] * wz * wy * wx)
    if not idxs:
        return np.zeros(0, np.int64), np.zeros(0, f32)
    return np.concatenate([i.reshape(-1) for i in idxs]), np.concatenate([v.reshape(-1) for v in vals]).astype(f32)


def to_fixed(v):
    """int64 2^-52 fixed point of float32 addends (nerf_to_fixed): |v| <= 256 rounds half to even; NaN / Inf -> 2^61;
    other |v| > 256 -> +-(2^60 + 2^59)."""
    v = np.asarray(v, dtype=f32)
    ok = np.abs(v) <= f32(256)
    q = np.rint(np.where(ok, v, f32(0)).astype(np.float64) * 2.0 ** FIX_SHIFT).astype(np.int64)
    sat = np.where(v > 0, np.int64(FIX_SATURATED), np.int64(-FIX_SATURATED))
    bad = np.where(np.isfinite(v), sat, np.int64(FIX_POISON))
    return np.where(ok, q, bad).astype(np.int64)


def scatter_fixed(idx, q, size, prefill=None):
    """prefill + the exact int64 sum of the fixed-point addends q per entry, wrapping mod 2^64 (integer addition is associative:
    any order, grouping or schedule gives this)."""
    out = np.zeros(size, np.int64) if prefill is None else np.array(prefill, dtype=np.int64, copy=True)
    if len(idx):
        order = np.argsort(idx, kind="stable")
        si, sq = idx[order], q[order]
        starts = np.flatnonzero(np.r_[True, si[1:] != si[:-1]])
        out[si[starts]] += np.add.reduceat(sq, starts)
    return out


def scatter_f64(idx, v, size):
    """float64 sum, sum of |addend| and addend count per entry (bounds of the float-atomic scatter)."""
    v = np.asarray(v, dtype=np.float64)
    return (np.bincount(idx, weights=v, minlength=size), np.bincount(idx, weights=np.abs(v), minlength=size),
            np.bincount(idx, minlength=size))


def _powf():
    path = ctypes.util.find_library("m")
    if path is None:
        return lambda a, b: np.power(f32(a), f32(b))
    fn = ctypes.CDLL(path).powf
    fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    return lambda a, b: f32(fn(float(a), float(b)))


powf = _powf()


def bias_factors(b1, b2, bias_correction, step):
    """c1, c2 as the host code computes them: 1 / (1 - powf(beta, step)) in float32."""
    if not bias_correction:
        return ONE, ONE
    return (ONE / (ONE - powf(f32(b1), f32(step))), ONE / (ONE - powf(f32(b2), f32(step))))


def fixed_grad(a, gscale):
    """float32 gradient of int64 accumulators (adam_kernel): float32(float64(a) 2^-52) * gscale, NaN outside (-2^60, 2^60)."""
    a = np.asarray(a, dtype=np.int64)
    g = (a.astype(np.float64) * 2.0 ** -FIX_SHIFT).astype(f32) * f32(gscale)
    return np.where((a <= -(1 << 60)) | (a >= (1 << 60)), f32(np.nan), g).astype(f32)


def adam_ex(p, g, m, v, lr, b1, b2, eps, c1, c2, gscale, fixed=False):
    """(p, m, v) after one step of adam_kernel; g float32 (scaled by gscale here) or int64 accumulators."""
    p, m, v = (np.asarray(t, dtype=f32) for t in (p, m, v))
    lr, b1, b2, eps, c1, c2 = (f32(t) for t in (lr, b1, b2, eps, c1, c2))
    gi = fixed_grad(g, gscale) if fixed else np.asarray(g, dtype=f32) * f32(gscale)
    mi = b1 * m + (ONE - b1) * gi
    vi = b2 * v + (ONE - b2) * gi * gi
    pn = p - lr * (mi * c1) / (np.sqrt(vi * c2) + eps)
    return pn.astype(f32), mi.astype(f32), vi.astype(f32)


# ---- inputs that exhaust the combine kernel's probe window (HC_PROBES linear probes from slot (idx * 2654435761) >> 22)

def hc_slot(idx):
    return ((np.asarray(idx, dtype=np.uint32) * P1) >> np.uint32(22)).astype(np.int64)


def lattice_keys(res, T):
    """int64 [(res+1)^3] key of every lattice point (i, j, k) in [0, res]^3 (i fastest), the coordinates [.., 3]."""
    a = np.arange(res + 1, dtype=np.uint32)
    k, j, i = np.meshgrid(a, a, a, indexing="ij")
    ijk = np.stack([i.reshape(-1), j.reshape(-1), k.reshape(-1)], 1)
    return hash3(ijk[:, 0], ijk[:, 1], ijk[:, 2], T).astype(np.int64), ijk


def probe_lattice_points(res, T, count, below):
    """`count` lattice points (positions [count, 3] in [0, 1]) with pairwise distinct keys whose home slots are < `below`."""
    keys, ijk = lattice_keys(res, T)
    sel = np.flatnonzero(hc_slot(keys) < below)
    _, first = np.unique(keys[sel], return_index=True)
    sel = sel[np.sort(first)][:count]
    assert len(sel) == count, (len(sel), count)
    return ijk[sel].astype(f32) / f32(res)


def probe_edges(res, T, count, below):
    """`count` samples on y- or z-edges of the lattice (two coordinates on the lattice, the third at the middle of a cell):
    each touches the two keys of the edge's end points; 2 `count` pairwise distinct keys, all with home slots < `below`.
    Returns positions [count, 3] and the keys [2 count]."""
    keys, ijk = lattice_keys(res, T)
    R1 = res + 1
    ok = hc_slot(keys) < below
    cand = []
    for axis, stride in ((1, R1), (2, R1 * R1)):
        a = np.flatnonzero(ok & (ijk[:, axis] < res))
        a = a[ok[a + stride]]
        cand += [(int(x), int(x + stride), axis) for x in a]
    used, pos, got = set(), [], []
    for lo, hi, axis in cand:
        ka, kb = int(keys[lo]), int(keys[hi])
        if ka == kb or ka in used or kb in used:
            continue
        used |= {ka, kb}
        c = ijk[lo].astype(np.float64)
        c[axis] += 0.5
        pos.append(c / res)
        got += [ka, kb]
        if len(pos) == count:
            break
    assert len(pos) == count, (len(pos), count)
    return np.asarray(pos, dtype=f32), np.asarray(got, dtype=np.int64)


def probes_needed(keys, order):
    """Linear probing with no deletion (one chunk), keys inserted in `order`: probes each DISTINCT key needs to find its
    slot (a key seen before costs nothing new).  A key past HC_PROBES goes to the global table and claims no slot."""
    table = np.full(HC_CAP, -1, np.int64)
    out = {}
    for k in np.asarray(keys)[order]:
        k = int(k)
        if k in out:
            continue
        s = int(hc_slot(k))
        for probe in range(HC_CAP):
            if table[s] in (-1, k):
                break
            s = (s + 1) & (HC_CAP - 1)
        out[k] = probe + 1
        if probe < HC_PROBES:
            table[s] = k
    return out
