"""Early ray termination without a GPU: the torch reference of tests/_ert_ref.py against a float64 brute-force composite at
eps = 0 and against the error bound of include/nerf_hip.h at eps > 0, and the argument checks of min_transmittance."""
import math

import pytest
import torch

from tests import _ert_ref as E
from tests import _march_ref as M
from tests import _occupancy_ref as O

LOG2_RES = 7
POS_SCALE, POS_OFFSET = 1.0 / 3.0, 0.5            # HashNeRF(bound=1.5)


def _rays(B, seed):
    """Rays from outside through the box, rays starting inside, axis-parallel and NaN rays."""
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(B, 3, generator=g) * 2 - 1) * 4.0
    d = torch.nn.functional.normalize((torch.rand(B, 3, generator=g) * 2 - 1) * 1.2 - o, dim=-1)
    nf = torch.tensor([[2.0, 6.0]]).expand(B, 2).clone()
    q = B // 8
    o[:q] = (torch.rand(q, 3, generator=g) - 0.5) * 2.0
    nf[:q, 0] = 0.0
    d[q:q + 4, 2] = 0.0
    o[q + 4:q + 6, 0] = float("nan")
    return torch.cat([o, d, nf, d], 1).float().contiguous()


def _scene(steps, seed, sigma_bias):
    rays = _rays(256, seed)
    g = torch.Generator().manual_seed(seed + 1)
    occ = torch.rand(1 << (3 * LOG2_RES), generator=g) < 0.5
    step = M.step_world(steps, 1.5)
    offs, rows, z, K = M.march(rays, 0.5, occ, LOG2_RES, POS_SCALE, POS_OFFSET, step, steps)
    raw = torch.rand(K, 4, generator=g)
    raw[:, 3] = torch.randn(K, generator=g) * 2.0 + sigma_bias
    return raw, z, offs, step


@pytest.mark.parametrize("white", [False, True])
def test_reference_at_eps_zero_is_the_full_composite(white):
    raw, z, offs, step = _scene(256, 1, 0.0)
    rgb, acc, depth, samples = E.fold(raw, z, offs, step, 0.0, white)
    w_rgb, w_acc, w_depth = M.composite(raw.double(), z.double(), offs, step, white)
    assert torch.equal(samples, offs[1:] - offs[:-1])
    assert float((rgb.double() - w_rgb).abs().max()) < 2e-5
    assert float((acc.double() - w_acc).abs().max()) < 2e-5
    assert float((depth.double() - w_depth).abs().max()) < 2e-4
    empty = (offs[1:] == offs[:-1])
    assert bool(empty.any()) and bool((acc[empty] == 0).all()) and bool((depth[empty] == 0).all())
    assert bool((rgb[empty] == (1.0 if white else 0.0)).all())


@pytest.mark.parametrize("eps", [1e-4, 1e-2, 0.5])
def test_reference_keeps_the_error_bound(eps):
    raw, z, offs, step = _scene(512, 2, 4.0)                 # dense: most rays saturate
    full = E.fold(raw, z, offs, step, 0.0, True)
    rgb, acc, depth, samples = E.fold(raw, z, offs, step, eps, True)
    lens = offs[1:] - offs[:-1]
    assert bool((samples <= lens).all())
    stopped = samples < lens
    assert int(stopped.sum()) >= int((lens > 0).sum()) // 4
    # |d rgb| <= T_stop max |c - bg| < eps (bg = 1, c in [0, 1)), 0 <= acc_full - acc_eps < eps, with float rounding on top
    T_stop = E.transmittance_at_stop(raw, offs, step, samples)
    tol = 1e-5
    d_rgb = (rgb.double() - full[0].double()).abs().max(1).values
    assert bool((d_rgb <= torch.where(stopped, T_stop, torch.zeros_like(T_stop)) + tol).all())
    assert float(d_rgb.max()) < eps + tol
    d_acc = full[1].double() - acc.double()
    assert bool((d_acc >= -tol).all()) and bool((d_acc < eps + tol).all())
    assert bool((T_stop[stopped] < eps * (1 + 1e-5)).all())


def test_reference_edge_cases():
    step = M.step_world(1024, 1.5)
    offs = torch.tensor([0, 3, 6, 9, 9])
    raw = torch.rand(9, 4, generator=torch.Generator().manual_seed(3))
    z = torch.linspace(2.0, 3.0, 9)
    raw[1, 3] = float("inf")                                 # ray 0: opaque at its second sample
    raw[4, 3] = float("nan")                                 # ray 1: NaN
    rgb, acc, depth, samples = E.fold(raw, z, offs, step, 1e-4, True)
    assert bool(torch.isfinite(rgb[0]).all()) and int(samples[0]) == 2
    assert bool(torch.isnan(rgb[1]).all()) and bool(torch.isfinite(rgb[2]).all())
    assert rgb[3].tolist() == [1.0] * 3 and float(acc[3]) == 0.0 and int(samples[3]) == 0


def test_min_transmittance_argument_checks():
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    from nerf_meets_mlx_amd.engine.occupancy import check_min_transmittance
    assert check_min_transmittance(None) is None
    for ok in (0, 0.0, 1e-4, 0.5, 0.999999):
        assert check_min_transmittance(ok) == float(ok)
    for bad in (-1e-9, 1.0, 1.5, math.nan, math.inf, -math.inf, "0.1", True, [1e-4]):
        with pytest.raises(ValueError):
            check_min_transmittance(bad)
    # the trainer checks before touching a device: no GPU needed
    with pytest.raises(ValueError, match="march_steps"):
        NGPTrainer(None, None, None, occupancy_grid=True, min_transmittance=1e-4)
    for bad in (math.nan, 1.0, -0.5):
        with pytest.raises(ValueError, match="min_transmittance"):
            NGPTrainer(None, None, None, occupancy_grid=True, march_steps=256, min_transmittance=bad)
