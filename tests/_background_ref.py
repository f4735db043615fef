"""Torch reference of compositing over a background colour and of training on straight RGBA targets (a helper module for the tests,
not a conftest; csrc/composite_packed.hip nerf_composite_packed_*_bg / nerf_ert_finish_bg are the product).  include/nerf_hip.h
"background colour" states the rules; this module spells them out on top of the existing references:

  render      tests/_march_ref.composite without a background, then rgb = sum w c + (1 - acc) bg
  target      t = rgba[:3] a + bg (1 - a), a = rgba[3] (straight alpha)
  objective   MSE(rgb, t) + weight * mean_b L_b (tests/_distortion_ref.losses), gradients by float64 autograd
  fold        tests/_ert_ref.fold without a background, then rgb += (1 - acc) bg in float32
bg is [3] (one colour) or [B, 3] (one per ray).
"""
import torch

from tests import _distortion_ref as D
from tests import _ert_ref as E
from tests import _march_ref as M


def composite(raw: torch.Tensor, z: torch.Tensor, offsets, step: float, bg: torch.Tensor):
    """(rgb [B, 3], acc [B], depth [B]) in raw's dtype."""
    c, acc, depth = M.composite(raw, z, offsets, step, False)
    return c + (1.0 - acc)[:, None] * bg.to(raw.dtype), acc, depth


def target(rgba: torch.Tensor, bg: torch.Tensor) -> torch.Tensor:
    """t [B, 3] in rgba's dtype."""
    a = rgba[:, 3:4]
    return rgba[:, :3] * a + bg.to(rgba.dtype) * (1.0 - a)


def objective_backward(raw, z, offsets, rays, step: float, march_steps: int, rgba, bg, weight: float = 0.0):
    """(mse, mean_b L_b, d_raw [K, 4], rgb [B, 3]) in float64: d_raw is the autograd gradient of mse + weight * mean_b L_b
    (weight 0: the plain training form; rays is not read then)."""
    r = raw.detach().double().requires_grad_(True)
    rgb, _, _ = composite(r, z.double(), offsets, step, bg.double())
    mse = ((rgb - target(rgba.double(), bg.double())) ** 2).mean()
    dist = D.losses(r, z, offsets, rays, step, march_steps).mean() if weight else r.new_zeros(())
    (mse + weight * dist).backward()
    return mse.detach(), dist.detach(), r.grad, rgb.detach()


def acc_adjoint(raw, z, offsets, step: float, rgba, bg):
    """(g [B, 3], gacc [B]) in float64 by autograd: d mse / d (sum w c) and d mse / d acc of every ray."""
    r = raw.detach().double()
    c, acc, _ = M.composite(r, z.double(), offsets, step, False)
    c, acc = c.detach().requires_grad_(True), acc.detach().requires_grad_(True)
    rgb = c + (1.0 - acc)[:, None] * bg.double()
    mse = ((rgb - target(rgba.double(), bg.double())) ** 2).mean()
    g, gacc = torch.autograd.grad(mse, [c, acc])
    return g, gacc


def fold(raw, z, offsets, step: float, eps: float, bg: torch.Tensor):
    """(rgb [B, 3], acc [B], depth [B], samples [B]) in float32: tests/_ert_ref.fold over bg."""
    c, acc, depth, samples = E.fold(raw, z, offsets, step, eps, False)
    one = torch.tensor(1.0, dtype=torch.float32, device=c.device)
    return c + (one - acc)[:, None] * bg.float().to(c.device), acc, depth, samples
