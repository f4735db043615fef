"""Distortion regulariser, host side (no GPU): the prefix-sum form the kernels use against the O(n^2) float64 definition of
tests/_distortion_ref.py, the properties of L_b, NGPTrainer's argument checks and the argument checks of the two C entry points."""
import ctypes as C

import pytest
import torch

from tests import _distortion_ref as D
from tests import _march_ref as M

S = 1024
STEP = M.step_world(S, 1.5)
SEGMENTS = [1, 2, 63, 64, 65, 300, 1024]


def _ray(n, seed, saturated):
    """(w [n], u [n]) in float32 of a thin (acc well below 1) or a saturated ray with n sorted samples."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.rand(n, 4, generator=g)
    raw[:, 3] = torch.randn(n, generator=g) * 2.0 + (6.0 if saturated else -4.0)
    z = torch.sort(torch.rand(n, generator=g) * 3.0 + 2.5).values
    w = D.weights(raw, STEP)
    u = (z - z[0]) * (torch.tensor(1.0) / (torch.tensor(float(S)) * torch.tensor(STEP)))
    return raw, z, w, u


@pytest.mark.parametrize("saturated", [False, True])
@pytest.mark.parametrize("n", SEGMENTS)
def test_prefix_sum_form_in_float32_matches_the_definition_in_float64(n, saturated):
    """Same float32 w and u on both sides, so only the summation order and float32 rounding differ.  Bounds: 3e-6 of the
    gradient's scale (3e-7 measured for this form on the CPU, times 10) and 2e-6 relative in L_b (2e-7 measured, times 10)."""
    _, _, w, u = _ray(n, 100 + n, saturated)
    L, g = D.prefix_f32(w, u, S)
    wL, wg = D.ray_loss(w.double(), u.double(), S), D.ray_grad(w.double(), u.double(), S)
    eg = float((g.double() - wg).abs().max()) / float(wg.abs().max())
    eL = abs(float(L) - float(wL)) / float(wL)
    print(f"\nn={n} saturated={saturated}: acc={float(w.sum()):.4f} L={float(wL):.3e} grad err {eg:.1e} L err {eL:.1e}")
    assert float(w.sum()) < 0.9 if not saturated else (n == 1 or float(w.sum()) > 0.9)
    assert eg <= 3e-6, eg
    assert eL <= 2e-6, eL


def test_the_double_sum_gradient_is_the_autograd_gradient():
    _, _, w, u = _ray(65, 7, False)
    wd = w.double().requires_grad_(True)
    D.ray_loss(wd, u.double(), S).backward()
    assert torch.allclose(wd.grad, D.ray_grad(w.double(), u.double(), S), rtol=1e-12, atol=0)


def test_properties_of_the_ray_loss():
    raw, z, w, u = _ray(300, 3, False)
    rays = torch.zeros(1, 11)
    rays[0, 3:6] = torch.tensor([0.6, 0.0, 0.8])                 # |d| = 1
    offs = [0, 300]
    L = D.losses(raw.double(), z, offs, rays, STEP, S)
    assert float(L[0]) > 0.0
    # the reference's weights are packed compositing's
    _, acc, _ = M.composite(raw.double(), z.double(), offs, STEP, False)
    assert abs(float(D.weights(raw.double(), STEP).sum()) - float(acc[0])) < 1e-15
    # one sample: (delta / 3) w^2
    L1 = D.losses(raw[:1].double(), z[:1], [0, 1], rays, STEP, S)
    assert abs(float(L1[0]) - float(D.weights(raw[:1].double(), STEP)[0]) ** 2 / (3.0 * S)) < 1e-18
    # no samples, a zero or a non-finite |d|: 0
    assert float(D.losses(raw.double(), z, [0, 0], rays, STEP, S)[0]) == 0.0
    for bad in (0.0, float("nan"), float("inf")):
        r = rays.clone()
        r[0, 3:6] = bad
        assert float(D.losses(raw.double(), z, offs, r, STEP, S)[0]) == 0.0
    # a constant added to z changes nothing; neither does scaling d by s and z by 1 / s (the same world points)
    zd, wd = z.double(), D.weights(raw.double(), STEP)
    La = D.ray_loss(wd, D.positions(zd + 1.25, 1.0, STEP, S), S)
    Lb = D.ray_loss(wd, D.positions(zd / 4.0, 4.0, STEP, S), S)
    L0 = D.ray_loss(wd, D.positions(zd, 1.0, STEP, S), S)
    assert abs(float(La) - float(L0)) < 1e-12 * float(L0) and abs(float(Lb) - float(L0)) < 1e-12 * float(L0)
    assert abs(float(L0) - float(L[0])) < 1e-12 * float(L0)
    # two equal clumps of weight: the further apart, the larger
    wc = torch.tensor([0.2, 0.2, 0.2, 0.2], dtype=torch.float64)
    near = D.ray_loss(wc, torch.tensor([0.0, 0.001, 0.10, 0.101], dtype=torch.float64), S)
    far = D.ray_loss(wc, torch.tensor([0.0, 0.001, 0.40, 0.401], dtype=torch.float64), S)
    one = D.ray_loss(wc, torch.tensor([0.0, 0.001, 0.002, 0.003], dtype=torch.float64), S)
    assert float(far) > float(near) > float(one) > 0.0


def test_objective_backward_leaves_the_colour_columns_to_the_mse():
    raw, z, _, _ = _ray(65, 5, False)
    rays = torch.zeros(1, 11)
    rays[0, 3:6] = torch.tensor([0.0, 0.6, 0.8])
    offs = [0, 65]
    rgb, _, _ = M.composite(raw.double(), z.double(), offs, STEP, True)
    mse, dist, d, _ = D.objective_backward(raw, z, offs, rays, STEP, S, rgb, True, 0.5)
    assert float(mse) < 1e-30 and float(dist) > 0.0
    assert float(d[:, :3].abs().max()) < 1e-15 and float(d[:, 3].abs().max()) > 0.0
    _, wd = M.mse_backward(raw, offs, STEP, torch.zeros(1, 3), True)
    _, _, d0, _ = D.objective_backward(raw, z, offs, rays, STEP, S, torch.zeros(1, 3), True, 0.0)
    assert torch.allclose(d0, wd, rtol=1e-12, atol=0)            # weight 0: the packed MSE backward


def test_trainer_checks_distortion_weight():
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    from nerf_meets_mlx_amd.engine.occupancy import check_distortion_weight
    assert check_distortion_weight(None) is None
    assert check_distortion_weight(1e-2) == 1e-2 and check_distortion_weight(1) == 1.0
    for bad in (0, 0.0, -1e-2, float("nan"), float("inf"), float("-inf"), "0.01", True):
        with pytest.raises(ValueError, match="distortion_weight"):
            check_distortion_weight(bad)
        with pytest.raises(ValueError, match="distortion_weight"):
            NGPTrainer(None, None, None, device="cpu", occupancy_grid=True, march_steps=64, distortion_weight=bad)
    with pytest.raises(ValueError, match="march_steps"):         # without the march
        NGPTrainer(None, None, None, device="cpu", distortion_weight=1e-2)
    with pytest.raises(ValueError, match="march_steps"):
        NGPTrainer(None, None, None, device="cpu", occupancy_grid=True, distortion_weight=1e-2)


def test_distortion_entry_points_check_their_arguments():
    from nerf_meets_mlx_amd import _native as N
    lib = N.lib()
    p, odd = C.c_void_p(16), C.c_void_p(20)
    OK, E_NULL, E_SHAPE = 0, -1, -2
    fwd, bwd = lib.nerf_composite_packed_distortion, lib.nerf_composite_packed_mse_dist_backward
    # (raw, z, offsets, rays, B, K, step_world, march_steps, white, rgb, acc, depth, dist, stream)
    assert fwd(p, p, p, p, 4, 8, 0.01, 0, 1, p, p, p, p, None) == E_SHAPE
    assert fwd(p, p, p, p, 4, 8, 0.01, 1025, 1, p, p, p, p, None) == E_SHAPE
    assert fwd(p, p, p, p, 4, 8, 0.0, 64, 1, p, p, p, p, None) == E_SHAPE
    assert fwd(p, p, p, p, 4, 8, -1.0, 64, 1, p, p, p, p, None) == E_SHAPE
    assert fwd(p, p, p, p, -1, 8, 0.01, 64, 1, p, p, p, p, None) == E_SHAPE
    assert fwd(odd, p, p, p, 4, 8, 0.01, 64, 1, p, p, p, p, None) == E_SHAPE
    assert fwd(None, None, None, None, 0, 0, 0.01, 64, 1, None, None, None, None, None) == OK
    assert fwd(None, None, None, None, 0, 0, 0.01, 0, 1, None, None, None, None, None) == E_SHAPE      # checked before B = 0
    for i in (0, 1, 2, 3, 9, 12):                               # raw, z, offsets, rays, rgb, dist
        a = [p, p, p, p, 4, 8, 0.01, 64, 1, p, p, p, p, None]
        a[i] = None
        assert fwd(*a) == E_NULL, i
    assert fwd(None, None, None, p, 4, 0, 0.01, 64, 1, p, None, None, p, None) == E_NULL               # K = 0: offsets still needed
    # (raw, z, offsets, rays, B, K, step_world, march_steps, white, target, grad_scale, dist_weight, loss, dist, rgb, d_raw, stream)
    assert bwd(p, p, p, p, 4, 8, 0.01, 0, 1, p, 1.0, 0.01, p, p, p, p, None) == E_SHAPE
    assert bwd(p, p, p, p, 4, 8, 0.01, 2048, 1, p, 1.0, 0.01, p, p, p, p, None) == E_SHAPE
    assert bwd(p, p, p, p, 4, 8, 0.0, 64, 1, p, 1.0, 0.01, p, p, p, p, None) == E_SHAPE
    for w in (-0.01, float("nan"), float("inf")):
        assert bwd(p, p, p, p, 4, 8, 0.01, 64, 1, p, 1.0, w, p, p, p, p, None) == E_SHAPE, w
    assert bwd(odd, p, p, p, 4, 8, 0.01, 64, 1, p, 1.0, 0.01, p, p, p, p, None) == E_SHAPE
    assert bwd(p, p, p, p, 4, 8, 0.01, 64, 1, p, 1.0, 0.01, p, p, p, odd, None) == E_SHAPE
    assert bwd(None, None, None, None, 0, 0, 0.01, 64, 1, None, 1.0, 0.01, None, None, None, None, None) == OK
    assert bwd(None, None, None, None, 0, 0, 0.01, 64, 1, None, 1.0, -1.0, None, None, None, None, None) == E_SHAPE
    for i in (0, 1, 2, 3, 9, 15):                               # raw, z, offsets, rays, target, d_raw
        a = [p, p, p, p, 4, 8, 0.01, 64, 1, p, 1.0, 0.01, p, p, p, p, None]
        a[i] = None
        assert bwd(*a) == E_NULL, i
    assert lib.nerf_abi_version() == 3
