"""Torch reference of the occupancy-grid rules (a helper module for the tests, not a conftest; engine/occupancy.py is the product).

Every function works on CPU or device tensors and spells out the arithmetic the kernels are held to:
  merge     density = where(r > d * 0.95, r, d * 0.95), r = where(sigma > 0, sigma, 0)     (float32, bit-exact)
  finalize  thr = min(thr_cap, float32(mean_f64(density))), bit = density > thr          (the mean may differ in the last ulp)
  pack      bit c is bit (c & 31) of int32 word c >> 5
  cell      u = (o + z d) * pos_scale + pos_offset per axis (float32, one rounding per op), cell = floor(u R) when every u is in
            [0, 1), index ix + R (iy + R iz); outside: empty
  points    the jittered point of every cell, bit for bit (numpy; see points())
  lookup    occupied_words: the bit of a cell straight from the packed words, so that a 1024^3 grid needs its 128 MiB of words only
"""
import numpy as np
import torch


def merge(density: torch.Tensor, sigma: torch.Tensor, decay: float = 0.95) -> torch.Tensor:
    d = density * torch.tensor(decay, dtype=torch.float32, device=density.device)
    r = torch.where(sigma > 0, sigma, torch.zeros_like(sigma))
    return torch.where(r > d, r, d)


def threshold(density: torch.Tensor, thr_cap: float) -> torch.Tensor:
    mean = density.double().mean().float()
    return torch.minimum(mean, torch.tensor(thr_cap, dtype=torch.float32, device=density.device))


def occupancy(density: torch.Tensor, thr: torch.Tensor) -> torch.Tensor:
    return density > thr


def pack(occ: torch.Tensor) -> torch.Tensor:
    """bool [R^3] -> int32 [R^3 / 32]."""
    b = occ.reshape(-1, 32).to(torch.int64)
    w = (b << torch.arange(32, dtype=torch.int64, device=occ.device)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack(bits: torch.Tensor) -> torch.Tensor:
    """int32 [R^3 / 32] -> bool [R^3]."""
    w = bits.to(torch.int64) & 0xFFFFFFFF
    return ((w[:, None] >> torch.arange(32, dtype=torch.int64, device=bits.device)) & 1).reshape(-1).bool()


def unit_coords(rays: torch.Tensor, z: torch.Tensor, pos_scale: float, pos_offset: float) -> torch.Tensor:
    """[B, n, 3] float32 unit-cube coordinates with the kernels' roundings."""
    s = torch.tensor(pos_scale, dtype=torch.float32, device=z.device)
    o = torch.tensor(pos_offset, dtype=torch.float32, device=z.device)
    p = rays[:, None, 0:3] + z[:, :, None] * rays[:, None, 3:6]
    return p * s + o


def cell_index(u: torch.Tensor, log2_res: int) -> torch.Tensor:
    """int64 [...] cell of unit-cube coordinates u [..., 3], -1 outside [0, 1)^3."""
    R = 1 << log2_res
    inside = ((u >= 0) & (u < 1)).all(-1)
    c = torch.floor(u * R).to(torch.int64).clamp(0, R - 1)
    idx = c[..., 0] + R * (c[..., 1] + R * c[..., 2])
    return torch.where(inside, idx, torch.full_like(idx, -1))


def occupied_words(words, c):
    """bool [...]: cell c (int64, -1: no cell, always empty) is occupied, read from the packed words (uint32 / int32 [R^3 / 32],
    numpy or torch) as the kernels read them: bit (c & 31) of word c >> 5."""
    if torch.is_tensor(words):
        cc = c.clamp(min=0)
        return (c >= 0) & (((words[cc >> 5].to(torch.int64) >> (cc & 31)) & 1) != 0)
    c = np.asarray(c, dtype=np.int64)
    cc = np.maximum(c, 0)
    return (c >= 0) & (((np.asarray(words)[cc >> 5].astype(np.int64) >> (cc & 31)) & 1) != 0)


def occupied(occ, c: torch.Tensor) -> torch.Tensor:
    """bool [...]: cell c (int64, -1: no cell) is occupied; occ is bool [R^3], or the packed words (occupied_words)."""
    if torch.is_tensor(occ) and occ.dtype == torch.bool:
        return (c >= 0) & occ[c.clamp(min=0)]
    if not torch.is_tensor(occ):
        return torch.from_numpy(occupied_words(occ, c.cpu().numpy())).to(c.device)
    return occupied_words(occ, c)


def keep_mask(rays, z, occ, log2_res: int, pos_scale: float, pos_offset: float) -> torch.Tensor:
    """bool [B, n]: the sample's cell exists and is occupied.  occ: bool [R^3], or the packed words."""
    return occupied(occ, cell_index(unit_coords(rays, z, pos_scale, pos_offset), log2_res))


# ---- the jittered points of nerf_occ_points (include/nerf_hip.h; csrc/occupancy.hip occ_points_kernel), in numpy
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def mix64(z):
    """The splitmix64 finaliser on uint64 (array or scalar), with wrap-around."""
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64))
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _cell_1d(u, R):
    """The cell of a unit-cube coordinate on one axis (float32 [N]), -1 outside [0, 1) (NaN included)."""
    with np.errstate(invalid="ignore"):
        inside = (u >= np.float32(0)) & (u < np.float32(1))
        c = np.floor(np.where(inside, u, np.float32(0)) * np.float32(R)).astype(np.int64)      # R a power of two: exact
    return np.where(inside, c, -1)


def points(log2_res: int, cell0: int, count: int, seed: int, update: int, pos_scale: float, pos_offset: float):
    """(p float32 [count, 3], fallback bool [count, 3]): the point of every cell of [cell0, cell0 + count) and where it is the
    cell centre instead of the jittered point.  float32 with one rounding per operation (no contraction, IEEE division):
      key = mix64(seed ^ mix64(update + 0x632BE59BD9B4E019))
      h = mix64(key + (3 c + a + 1) * 0x9E3779B97F4A7C15) per axis a of cell c = ix + R (iy + R iz), all modulo 2^64
      u = float32(h >> 40) * 2^-24;  q = (float32(ci) + u) * (1 / R);  p = (q - pos_offset) / pos_scale
      when p * pos_scale + pos_offset is not in cell ci of the axis: the same with u = 0.5"""
    R = 1 << log2_res
    s, o = np.float32(pos_scale), np.float32(pos_offset)
    inv_R = np.float32(1.0) / np.float32(R)
    u64 = lambda v: np.uint64(int(v) & 0xFFFFFFFFFFFFFFFF)  # noqa: E731
    with np.errstate(over="ignore"):
        key = mix64(u64(seed) ^ mix64(u64(update) + np.uint64(0x632BE59BD9B4E019)))[0]
    c = np.arange(cell0, cell0 + count, dtype=np.int64)
    ci = [c & (R - 1), (c >> log2_res) & (R - 1), c >> (2 * log2_res)]
    cu = c.astype(np.uint64)
    p = np.empty((count, 3), dtype=np.float32)
    fallback = np.zeros((count, 3), dtype=bool)
    for a in range(3):
        with np.errstate(over="ignore"):
            h = mix64(key + (np.uint64(3) * cu + np.uint64(a + 1)) * np.uint64(0x9E3779B97F4A7C15))
        u = (h >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
        cf = ci[a].astype(np.float32)
        pa = ((cf + u) * inv_R - o) / s
        centre = ((cf + np.float32(0.5)) * inv_R - o) / s
        fb = _cell_1d(pa * s + o, R) != ci[a]
        p[:, a] = np.where(fb, centre, pa)
        fallback[:, a] = fb
    return p, fallback
