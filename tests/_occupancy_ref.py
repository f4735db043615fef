"""Torch reference of the occupancy-grid rules (a helper module for the tests, not a conftest; engine/occupancy.py is the product).

Every function works on CPU or device tensors and spells out the arithmetic the kernels are held to:
  merge     density = where(r > d * 0.95, r, d * 0.95), r = where(sigma > 0, sigma, 0)     (float32, bit-exact)
  finalize  thr = min(thr_cap, float32(mean_f64(density))), bit = density > thr          (the mean may differ in the last ulp)
  pack      bit c is bit (c & 31) of int32 word c >> 5
  cell      u = (o + z d) * pos_scale + pos_offset per axis (float32, one rounding per op), cell = floor(u R) when every u is in
            [0, 1), index ix + R (iy + R iz); outside: empty
"""
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


def keep_mask(rays, z, occ: torch.Tensor, log2_res: int, pos_scale: float, pos_offset: float) -> torch.Tensor:
    """bool [B, n]: the sample's cell exists and is occupied."""
    c = cell_index(unit_coords(rays, z, pos_scale, pos_offset), log2_res)
    return (c >= 0) & occ[c.clamp(min=0)]
