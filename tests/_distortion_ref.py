"""Torch reference of the distortion regulariser (a helper module for the tests, not a conftest; csrc/composite_packed.hip
nerf_composite_packed_distortion / _mse_dist_backward are the product).  include/nerf_hip.h "distortion regulariser" states the
rules; this module spells them out:

  weights     tests/_march_ref.composite's: sigma = trunc_exp(raw[3]), x = sigma step, alpha = 1 - exp(-x), T = exp(-exclusive
              cumsum x), w = alpha T
  positions   u_k = (z_k - z_first) |d| / (S step), |d| the march's norm (float products, double square root rounded to float)
  L_b         sum_i sum_j w_i w_j |u_i - u_j| + (1 / (3 S)) sum_i w_i^2 by the O(n^2) definition in float64; 0 for a ray without
              samples or with a zero / non-finite |d|
  objective   MSE + weight * mean_b L_b, gradients by float64 autograd through _march_ref.TruncExp
  prefix_f32  the kernel's prefix-sum form in float32, one rounding per operation in the header's order, with sequential sums
              where the kernel has wave scans (only the summation order differs)
"""
import torch

from tests import _march_ref as M


def weights(r: torch.Tensor, step: float) -> torch.Tensor:
    """w [n] of one ray's raw rows r [n, 4], in r's dtype (the lines of _march_ref.composite)."""
    x = M.trunc_exp(r[:, 3]) * step
    alpha = 1.0 - torch.exp(-x)
    excl = torch.cat([x.new_zeros(1), torch.cumsum(x, 0)[:-1]])
    return alpha * torch.exp(-excl)


def dnorm(rays: torch.Tensor) -> torch.Tensor:
    """|d| [B] of rays [B, 11] in float32, the march's way."""
    d = rays[:, 3:6].float()
    return torch.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).double()).float()


def positions(z: torch.Tensor, dn: float, step: float, march_steps: int) -> torch.Tensor:
    """u [n] in float64 of one ray's depths z [n] (n >= 1)."""
    z = z.double()
    return (z - z[0]) * float(dn) / (march_steps * float(step))


def ray_loss(w: torch.Tensor, u: torch.Tensor, march_steps: int) -> torch.Tensor:
    """L_b by the O(n^2) definition (w, u float64 [n])."""
    return (w[:, None] * w[None, :] * (u[:, None] - u[None, :]).abs()).sum() + (w * w).sum() / (3.0 * march_steps)


def ray_grad(w: torch.Tensor, u: torch.Tensor, march_steps: int) -> torch.Tensor:
    """dL_b / dw [n] by the O(n^2) definition."""
    return 2.0 * (w[None, :] * (u[:, None] - u[None, :]).abs()).sum(1) + 2.0 * w / (3.0 * march_steps)


def losses(raw: torch.Tensor, z: torch.Tensor, offsets, rays: torch.Tensor, step: float, march_steps: int) -> torch.Tensor:
    """L [B] in raw's dtype (float64 for the reference; differentiable in raw)."""
    offs = [int(v) for v in offsets]
    dn = dnorm(rays)
    out = []
    for b in range(len(offs) - 1):
        r, zz = raw[offs[b]:offs[b + 1]], z[offs[b]:offs[b + 1]]
        if r.shape[0] == 0 or not (bool(torch.isfinite(dn[b])) and float(dn[b]) > 0.0):
            out.append(raw.new_zeros(()))
            continue
        out.append(ray_loss(weights(r, step), positions(zz, dn[b], step, march_steps).to(raw.dtype), march_steps))
    return torch.stack(out) if out else raw.new_zeros(0)


def objective_backward(raw, z, offsets, rays, step: float, march_steps: int, target, white: bool, weight: float):
    """(mse, mean_b L_b, d_raw [K, 4], rgb [B, 3]) in float64: d_raw is the autograd gradient of mse + weight * mean_b L_b."""
    r = raw.detach().double().requires_grad_(True)
    rgb, _, _ = M.composite(r, z.double(), offsets, step, white)
    mse = ((rgb - target.double()) ** 2).mean()
    dist = losses(r, z, offsets, rays, step, march_steps).mean()
    (mse + weight * dist).backward()
    return mse.detach(), dist.detach(), r.grad, rgb.detach()


def prefix_f32(w: torch.Tensor, u: torch.Tensor, march_steps: int):
    """(L_b, dL_b/dw [n]) of float32 w, u [n] by the header's prefix-sum form, every operation rounded to float32."""
    w, u = w.float(), u.float()
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    wu = w * u
    zero = torch.zeros(1, dtype=torch.float32)
    cw, cu = torch.cumsum(w, 0), torch.cumsum(wu, 0)
    Wl, Ul = torch.cat([zero, cw[:-1]]), torch.cat([zero, cu[:-1]])
    W, U = cw[-1], cu[-1]
    c1 = (f(1.0) / f(float(march_steps))) / f(3.0)
    L = f(2.0) * (w * (u * Wl - Ul)).sum() + c1 * (w * w).sum()
    inter = u * ((f(2.0) * Wl + w) - W) - ((f(2.0) * Ul + wu) - U)
    return L, f(2.0) * inter + (f(2.0) * c1) * w
