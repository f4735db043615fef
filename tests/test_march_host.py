"""Occupancy-guided ray march, host side (no GPU): the torch reference of tests/_march_ref.py checked against plain fixed-step
sampling, the constructor's ValueError cases, and the argument checks of the new C entry points."""
import ctypes as C
import math

import pytest
import torch

from tests import _march_ref as M
from tests import _occupancy_ref as O

SCALE, OFFSET = float(torch.tensor(1.0 / 3.0, dtype=torch.float32)), 0.5     # HashNeRF(bound=1.5)


def _rays(B, seed, inside=False):
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(B, 3, generator=g) - 0.5) * (1.0 if inside else 6.0)
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1)
    nf = torch.tensor([[0.0, 4.0]]).expand(B, 2) if inside else torch.tensor([[2.0, 6.0]]).expand(B, 2)
    return torch.cat([o, d, nf, d], 1).float().contiguous()


def test_step_world():
    assert M.step_world(1024, 1.5) == float(torch.tensor(math.sqrt(3) / 1024 * 3.0, dtype=torch.float32))
    from nerf_meets_mlx_amd.engine.occupancy import march_step_world
    for s in (1, 64, 512, 1024):
        assert march_step_world(s, 1.5) == M.step_world(s, 1.5)


def test_full_grid_is_fixed_step_sampling_of_the_clipped_interval():
    rays = _rays(200, 1)
    step = M.step_world(256, 1.5)
    t0, t1, dt, ok = M.interval(rays, SCALE, OFFSET, step)
    assert 20 < int(ok.sum()) < 200                              # some rays miss the box
    full = torch.ones(2 ** 21, dtype=torch.bool)
    offs, rows, z, K = M.march(rays, 0.25, full, 7, SCALE, OFFSET, step, 256)
    none_, _, z2, K2 = M.march(rays, 0.25, None, 7, SCALE, OFFSET, step, 256)
    assert K == K2 and torch.equal(offs, none_) and torch.equal(z, z2)         # bits == NULL: every cell of the box
    assert K > 0 and rows.shape == (K, 11)
    for b in range(200):
        seg = z[offs[b]:offs[b + 1]].double()
        if not bool(ok[b]):
            assert seg.numel() == 0
            continue
        assert torch.equal(rows[offs[b]:offs[b + 1]], rays[b].expand(seg.numel(), 11))
        # plain fixed-step sampling of [t0, t1]: t0 + (k + j) dt, every step inside the box (rounding at the faces aside)
        n_plain = math.ceil((float(t1[b]) - float(t0[b])) / float(dt[b]) - 0.25)
        assert abs(seg.numel() - n_plain) <= 2, (b, seg.numel(), n_plain)
        if seg.numel():
            k = torch.arange(seg.numel(), dtype=torch.float64) + (seg[0] - float(t0[b])) / float(dt[b])
            assert torch.allclose(seg, float(t0[b]) + k * float(dt[b]), rtol=0, atol=1e-5)
            assert abs((float(seg[0]) - float(t0[b])) / float(dt[b]) - round((float(seg[0]) - float(t0[b])) / float(dt[b]) - 0.25)
                       - 0.25) < 1e-3
            assert float(seg[-1]) < float(t1[b])
        # the chord bound: never more than march_steps samples
        assert seg.numel() <= 256


def test_one_cell_grid_keeps_only_depths_in_that_cell():
    rays = _rays(300, 2, inside=True)
    c_w = (64.5 / 128 - 0.5) * 3.0                               # world centre of cell (64, 64, 64)
    aim = torch.nn.functional.normalize(c_w - rays[:150, 0:3], dim=-1)     # half the rays through the cell's centre
    rays[:150, 3:6] = aim
    rays[:150, 8:11] = aim
    step = M.step_world(1024, 1.5)
    cell = 64 + 128 * (64 + 128 * 64)
    occ = torch.zeros(2 ** 21, dtype=torch.bool)
    occ[cell] = True
    offs, rows, z, K = M.march(rays, 0.5, occ, 7, SCALE, OFFSET, step, 1024)
    assert K > 0
    c = O.cell_index(O.unit_coords(rows, z[:, None], SCALE, OFFSET)[:, 0], 7)
    assert bool((c == cell).all())
    # every step of the full march that lies in the cell is kept
    _, rows_f, z_f, _ = M.march(rays, 0.5, None, 7, SCALE, OFFSET, step, 1024)
    cf = O.cell_index(O.unit_coords(rows_f, z_f[:, None], SCALE, OFFSET)[:, 0], 7)
    assert int((cf == cell).sum()) == K


def test_cap_and_degenerate_rays():
    rays = _rays(50, 3, inside=True)
    step = M.step_world(1, 1.5)
    offs, _, _, K = M.march(rays, 0.0, None, 7, SCALE, OFFSET, step, 1)
    assert bool(((offs[1:] - offs[:-1]) <= 1).all()) and K > 0
    bad = rays[:4].clone()
    bad[0, 3] = 0.0                                              # axis-parallel
    bad[1, 0] = float("nan")
    bad[2, 6] = float("inf")
    bad[3, 0:3] = torch.tensor([10.0, 10.0, 10.0])               # misses the box (o outside, d random)
    bad[3, 3:6] = torch.tensor([1.0, 0.5, 0.25])
    offs, _, _, K = M.march(bad, 0.5, None, 7, SCALE, OFFSET, M.step_world(64, 1.5), 64)
    assert K == 0 and offs.tolist() == [0] * 5


def test_packed_composite_reference():
    raw = torch.tensor([[0.2, 0.4, 0.6, 100.0], [0.9, 0.9, 0.9, 1.0]], dtype=torch.float64)
    offs = torch.tensor([0, 0, 2])
    rgb, acc, depth = M.composite(raw, torch.tensor([2.0, 3.0]), offs, 0.01, True)
    assert rgb[0].tolist() == [1.0, 1.0, 1.0] and float(acc[0]) == 0.0 and float(depth[0]) == 0.0     # no samples: background
    assert abs(float(acc[1]) - 1.0) < 1e-12 and torch.allclose(rgb[1], raw[0, :3])                     # opaque first sample
    # trunc_exp: the backward is exp(min(x, 15))
    x = torch.tensor([0.0, 15.0, 40.0], dtype=torch.float64, requires_grad=True)
    M.trunc_exp(x).sum().backward()
    assert torch.allclose(x.grad, torch.exp(torch.tensor([0.0, 15.0, 15.0], dtype=torch.float64)))
    loss, d = M.mse_backward(raw.float(), offs, 0.01, torch.zeros(2, 3), False)
    assert d.shape == (2, 4) and bool(torch.isfinite(d).all()) and float(loss) > 0


def test_constructor_value_errors():
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    for kw in ({"march_steps": 64},                              # without occupancy_grid
               {"occupancy_grid": True, "march_steps": 0},
               {"occupancy_grid": True, "march_steps": 1025},
               {"occupancy_grid": True, "march_steps": 64.0},
               {"occupancy_grid": True, "march_steps": 64, "bound": None}):
        with pytest.raises(ValueError):
            NGPTrainer(None, None, None, device="cpu", **kw)
    from nerf_meets_mlx_amd.engine.occupancy import OccupancyGrid

    class Field:
        bound, pos_scale, pos_offset = 1.5, SCALE, OFFSET
    for bad in (0, 2048, -1):
        with pytest.raises(ValueError):
            OccupancyGrid(Field(), 2.0, 6.0, 64, device="cpu", march_steps=bad)
    g = OccupancyGrid(Field(), 2.0, 6.0, 64, device="cpu", march_steps=1024)
    assert g.step_world == M.step_world(1024, 1.5) and g.thr_cap == 0.01 / g.step_world
    assert OccupancyGrid(Field(), 2.0, 6.0, 64, device="cpu").thr_cap == 0.01 / (4.0 / 64)


def test_march_entry_points_check_their_arguments():
    from nerf_meets_mlx_amd import _native as N
    lib = N.lib()
    assert lib.nerf_occ_march_workspace_bytes(-1) == -1
    assert lib.nerf_occ_march_workspace_bytes(256) == 8 + 256 * 4
    assert lib.nerf_occ_march_workspace_bytes(257) == 16 + 1032
    p = C.c_void_p(16)
    assert lib.nerf_occ_march_count(p, 4, None, 0.5, None, 7, 1.0, 0.0, 0.01, 0, p, p, None) == -2       # march_steps 0
    assert lib.nerf_occ_march_count(p, 4, None, 0.5, None, 7, 1.0, 0.0, 0.01, 1025, p, p, None) == -2
    assert lib.nerf_occ_march_count(p, 4, None, 0.5, None, 7, 1.0, 0.0, 0.0, 64, p, p, None) == -2        # step 0
    assert lib.nerf_occ_march_count(None, 4, None, 0.5, None, 7, 1.0, 0.0, 0.01, 64, p, p, None) == -1
    assert lib.nerf_occ_march_write(p, 4, None, 0.5, None, 7, 1.0, 0.0, 0.01, 64, p, p, None, None, None) == -1
    assert lib.nerf_occ_merge_ex(None, None, 4, 0.95, 2, None) == -2
    assert lib.nerf_occ_merge_ex(None, None, 4, 0.95, 1, None) == -1
    assert lib.nerf_occ_merge_ex(None, None, 0, 0.95, 1, None) == 0
    assert lib.nerf_composite_packed_forward(None, None, None, 4, 0, 0.01, 1, None, None, None, None) == -1
    assert lib.nerf_composite_packed_forward(None, None, None, 4, 0, 0.0, 1, None, None, None, None) == -2
    assert lib.nerf_composite_packed_forward(None, None, None, 0, 0, 0.01, 1, None, None, None, None) == 0
    assert lib.nerf_composite_packed_mse_backward(None, None, 4, 0, 0.01, 1, None, 1.0, None, None, None, None) == -1
    assert lib.nerf_abi_version() == 3
