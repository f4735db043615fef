"""Torch reference of the occupancy-guided ray march and the packed compositing (a helper module for the tests, not a conftest;
engine/occupancy.py, csrc/occupancy.hip and csrc/composite_packed.hip are the product).  include/nerf_hip.h "ray march" and
"packed compositing" state the rules; this module spells them out:

  step_world  float32(sqrt(3) / march_steps * 2 bound), rounded once from double
  march       float32, one rounding per op in the header's order, so that every depth and every keep decision is the kernel's bit
              for bit: slab [t0, t1] of [near, far] with the box, dt = step_world / |d| (|d| a double sqrt rounded to float),
              z_k = t0 + (k + j) dt while z_k < t1 and k < 2 march_steps, kept when the cell (tests/_occupancy_ref.py) exists and is occupied, at most march_steps
  composite   sigma = trunc_exp(raw[3]) (exp; backward exp(min(x, 15))), x = sigma step_world, alpha = 1 - exp(-x),
              T = exp(-exclusive cumsum x), w = alpha T; rgb = sum w c (+ 1 - acc on white), acc = sum w, depth = sum w z
"""
import math

import torch

from tests import _occupancy_ref as O


def step_world(march_steps: int, bound: float) -> float:
    return float(torch.tensor(math.sqrt(3.0) / march_steps * 2.0 * bound, dtype=torch.float32))


def _f(v, like):
    return torch.tensor(v, dtype=torch.float32, device=like.device)


def interval(rays: torch.Tensor, pos_scale: float, pos_offset: float, step: float):
    """(t0 [B], t1 [B], dt [B], ok [B]) in float32."""
    rays = rays.float()
    s, off = _f(pos_scale, rays), _f(pos_offset, rays)
    lo, hi = (_f(0.0, rays) - off) / s, (_f(1.0, rays) - off) / s
    o, d = rays[:, 0:3], rays[:, 3:6]
    t0, t1 = rays[:, 6].clone(), rays[:, 7].clone()
    for a in range(3):
        ta, tb = (lo - o[:, a]) / d[:, a], (hi - o[:, a]) / d[:, a]
        t0 = torch.fmax(t0, torch.fmin(ta, tb))
        t1 = torch.fmin(t1, torch.fmax(ta, tb))
    dn = torch.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).double()).float()
    dt = _f(step, rays) / dn
    ok = torch.isfinite(rays[:, 0:8]).all(1) & (d != 0).all(1) & (t0 < t1) & (dt > 0)
    return t0, t1, dt, ok


def march(rays: torch.Tensor, jitter, occ, log2_res: int, pos_scale: float, pos_offset: float, step: float, march_steps: int):
    """(offsets [B + 1] int64, rows [K, 11], z [K], K).  jitter: float or float32 [B]; occ: bool [R^3] or the packed words
    (tests/_occupancy_ref.py occupied_words), or None (every cell of the box counts as occupied, the warm-up)."""
    rays = rays.float()
    B = rays.shape[0]
    j = jitter.float() if torch.is_tensor(jitter) else torch.full((B,), float(jitter), dtype=torch.float32, device=rays.device)
    t0, t1, dt, ok = interval(rays, pos_scale, pos_offset, step)
    ok = ok & torch.isfinite(j)
    k = torch.arange(2 * march_steps, dtype=torch.float32, device=rays.device)
    z = t0[:, None] + (k[None, :] + j[:, None]) * dt[:, None]                    # [B, 2 S]
    live = torch.cumprod((z < t1[:, None]).to(torch.int32), 1).bool() & ok[:, None]
    c = O.cell_index(O.unit_coords(rays, torch.where(live, z, torch.zeros_like(z)), pos_scale, pos_offset), log2_res)
    keep = live & (c >= 0)
    if occ is not None:
        keep = keep & O.occupied(occ, c)
    keep = keep & (torch.cumsum(keep.to(torch.int64), 1) <= march_steps)
    counts = keep.sum(1)
    offsets = torch.zeros(B + 1, dtype=torch.int64, device=rays.device)
    offsets[1:] = torch.cumsum(counts, 0)
    b_idx, _ = torch.nonzero(keep, as_tuple=True)
    return offsets, rays[b_idx], z[keep], int(offsets[-1])


class TruncExp(torch.autograd.Function):
    """exp forward; backward exp(min(x, 15)) (Instant-NGP)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(torch.clamp(x, max=15.0))


def trunc_exp(x):
    return TruncExp.apply(x)


def composite(raw: torch.Tensor, z: torch.Tensor, offsets, step: float, white: bool):
    """(rgb [B, 3], acc [B], depth [B]) of packed rays, in the dtype of raw (float64 for the autograd reference)."""
    offs = [int(v) for v in offsets]
    B = len(offs) - 1
    rgb, acc, depth = [], [], []
    for b in range(B):
        r, zz = raw[offs[b]:offs[b + 1]], z[offs[b]:offs[b + 1]].to(raw.dtype)
        x = trunc_exp(r[:, 3]) * step
        alpha = 1.0 - torch.exp(-x)
        excl = torch.cat([x.new_zeros(1), torch.cumsum(x, 0)[:-1]])
        w = alpha * torch.exp(-excl)
        c = (w[:, None] * r[:, :3]).sum(0)
        a = w.sum()
        if white:
            c = c + (1.0 - a)
        rgb.append(c)
        acc.append(a)
        depth.append((w * zz).sum())
    if B == 0:
        return raw.new_zeros(0, 3), raw.new_zeros(0), raw.new_zeros(0)
    return torch.stack(rgb), torch.stack(acc), torch.stack(depth)


def mse_backward(raw: torch.Tensor, offsets, step: float, target: torch.Tensor, white: bool):
    """(loss, d_raw [K, 4]) in float64 by autograd: loss = mean over B x 3 of (rgb - target)^2."""
    r = raw.detach().double().requires_grad_(True)
    z = torch.zeros(r.shape[0], dtype=torch.float64, device=r.device)
    rgb, _, _ = composite(r, z, offsets, step, white)
    loss = ((rgb - target.double()) ** 2).mean()
    loss.backward()
    return loss.detach(), r.grad
