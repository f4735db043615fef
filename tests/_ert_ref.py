"""Torch reference of early ray termination (a helper module for the tests, not a conftest; engine/occupancy.py render_ert and
csrc/composite_packed.hip nerf_ert_fold are the product).  include/nerf_hip.h "early ray termination" states the rules: the
samples are those of the one-shot march (tests/_march_ref.py), folded serially per ray in float32, one rounding per op:

  T = exp(-carry); T < eps terminates the ray (this sample and all later ones skipped; NaN T does not terminate)
  x = exp(raw[3]) * step_world, alpha = 1 - exp(-x), w = alpha * T
  r += w c_r, g += w c_g, b += w c_b, acc += w, depth += w z, carry += x, samples += 1
  rgb += (1 - acc) on a white background

The rays are folded side by side (sample i of every ray at once), each ray serially, so the arithmetic is the kernel's; only
torch's exp may differ from the device's expf in the last place.
"""
import torch

from tests import _march_ref as M
from tests import _occupancy_ref as O


def march_keep(rays: torch.Tensor, jitter, occ, log2_res: int, pos_scale: float, pos_offset: float, step: float,
               march_steps: int):
    """(keep [B, 2 S] bool, z [B, 2 S]): the keep decision and depth of every candidate k of the one-shot march
    (tests/_march_ref.py march, before packing), so that a resumed walk can be checked from any (k, kept)."""
    rays = rays.float()
    B = rays.shape[0]
    j = jitter.float() if torch.is_tensor(jitter) else torch.full((B,), float(jitter), dtype=torch.float32, device=rays.device)
    t0, t1, dt, ok = M.interval(rays, pos_scale, pos_offset, step)
    ok = ok & torch.isfinite(j)
    k = torch.arange(2 * march_steps, dtype=torch.float32, device=rays.device)
    z = t0[:, None] + (k[None, :] + j[:, None]) * dt[:, None]
    live = torch.cumprod((z < t1[:, None]).to(torch.int32), 1).bool() & ok[:, None]
    c = O.cell_index(O.unit_coords(rays, torch.where(live, z, torch.zeros_like(z)), pos_scale, pos_offset), log2_res)
    keep = live & (c >= 0)
    if occ is not None:                                      # bool [R^3], or the packed words
        keep = keep & O.occupied(occ, c)
    keep = keep & (torch.cumsum(keep.to(torch.int64), 1) <= march_steps)
    return keep, z


def fold(raw: torch.Tensor, z: torch.Tensor, offsets, step: float, eps: float, white: bool):
    """(rgb [B, 3], acc [B], depth [B], samples [B] int64) in float32 of packed rays: ray b owns raw [K, 4] / z [K] rows
    [offsets[b], offsets[b + 1])."""
    raw, z = raw.float().reshape(-1, 4), z.float().reshape(-1)
    offs = torch.as_tensor(offsets, dtype=torch.int64).to(raw.device)
    B = offs.numel() - 1
    lens = offs[1:] - offs[:-1]
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=raw.device)  # noqa: E731
    step_t, eps_t, one = f(step), f(eps), f(1.0)
    carry = torch.zeros(B, dtype=torch.float32, device=raw.device)
    c = torch.zeros(B, 3, dtype=torch.float32, device=raw.device)
    acc, depth = torch.zeros_like(carry), torch.zeros_like(carry)
    samples = torch.zeros(B, dtype=torch.int64, device=raw.device)
    term = torch.zeros(B, dtype=torch.bool, device=raw.device)
    for i in range(int(lens.max()) if B else 0):
        active = (i < lens) & ~term
        if not bool(active.any()):
            break
        T = torch.exp(-carry)
        stop = active & (T < eps_t)
        term |= stop
        go = active & ~stop
        k = torch.where(go, offs[:-1] + i, torch.zeros_like(offs[:-1]))
        rv, zk = raw[k], z[k]
        x = torch.exp(rv[:, 3]) * step_t
        alpha = one - torch.exp(-x)
        w = alpha * T
        c = torch.where(go[:, None], c + w[:, None] * rv[:, :3], c)
        acc = torch.where(go, acc + w, acc)
        depth = torch.where(go, depth + w * zk, depth)
        carry = torch.where(go, carry + x, carry)
        samples += go.to(torch.int64)
    if white:
        c = c + (one - acc)[:, None]
    return c, acc, depth, samples


def transmittance_at_stop(raw: torch.Tensor, offsets, step: float, samples: torch.Tensor) -> torch.Tensor:
    """float64 [B]: exp(-sum of x over the first samples[b] samples of ray b), the T at which the ray stopped (or its final T)."""
    raw = raw.double().reshape(-1, 4)
    offs = [int(v) for v in offsets]
    out = []
    for b in range(len(offs) - 1):
        x = torch.exp(raw[offs[b]:offs[b] + int(samples[b]), 3]) * step
        out.append(torch.exp(-x.sum()))
    return torch.stack(out) if out else raw.new_zeros(0)
