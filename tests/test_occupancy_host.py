"""Occupancy grid, host side (no GPU): the C ABI exports and sizes, argument checks, the scene-box requirement, and the torch
reference of tests/_occupancy_ref.py on the CPU (bit order, cell map)."""
import ctypes as C

import pytest
import torch

from tests import _occupancy_ref as R


def test_occupancy_entry_points_and_sizes():
    from nerf_meets_mlx_amd import _native as N
    lib = N.lib()
    assert lib.nerf_occ_finalize_workspace_bytes(7) == (128 ** 3 // 4096) * 8
    assert lib.nerf_occ_finalize_workspace_bytes(1) == -1 and lib.nerf_occ_finalize_workspace_bytes(11) == -1
    assert lib.nerf_occ_cull_workspace_bytes(4096, 64) == 256 * 8
    assert lib.nerf_occ_cull_workspace_bytes(37, 29) == 2 * 8            # 1073 samples: two workgroups of 1024
    assert lib.nerf_occ_cull_workspace_bytes(0, 64) == 0
    # shape / NULL checks fire before any device work
    assert lib.nerf_occ_points(11, 0, 1, 0, 0, 1.0, 0.0, None, None, None) == -2
    assert lib.nerf_occ_points(7, 128 ** 3, 1, 0, 0, 1.0, 0.0, C.c_void_p(8), C.c_void_p(8), None) == -2
    assert lib.nerf_occ_points(7, 0, 4, 0, 0, 1.0, 0.0, None, None, None) == -1
    assert lib.nerf_occ_merge(None, None, 4, 0.95, None) == -1
    assert lib.nerf_occ_finalize(None, 7, 0.16, None, None, None, None) == -1
    assert lib.nerf_occ_cull(None, None, 4, 4, None, 7, 1.0, 0.0, None, None, None, None, None, None, None) == -1
    assert lib.nerf_scatter_rows(None, None, 3, 4, None, 3, None) == -1
    assert lib.nerf_scatter_rows(None, None, 0, 4, None, 0, None) == 0
    assert lib.nerf_abi_version() == 3


def test_grid_refuses_world_coordinates():
    from nerf_meets_mlx_amd.engine.occupancy import OccupancyGrid

    class WorldField:                   # what HashNeRF(bound=None) exposes
        bound, pos_scale, pos_offset = None, 1.0, 0.0
    with pytest.raises(ValueError):
        OccupancyGrid(WorldField(), 2.0, 6.0, 64, device="cpu")


def test_reference_bit_order_and_cell_map():
    occ = torch.zeros(4 ** 3, dtype=torch.bool)
    occ[[0, 31, 32, 63]] = True
    bits = R.pack(occ)
    assert bits.dtype == torch.int32 and bits.tolist() == [1 - 2 ** 31, 1 - 2 ** 31]
    assert torch.equal(R.unpack(bits), occ)
    # scene box [-1.5, 1.5]^3 (pos_scale 1/3, offset 0.5), R = 4: a point at the box corner is cell 0, the far corner is outside
    rays = torch.tensor([[-1.5, -1.5, -1.5, 1.0, 0.0, 0.0, 0, 0, 1.0, 0.0, 0.0]])
    z = torch.tensor([[0.0, 0.75, 2.9, 3.0, float("nan")]])
    c = R.cell_index(R.unit_coords(rays, z, 1.0 / 3.0, 0.5), 2)
    assert c.tolist() == [[0, 1, 3, -1, -1]]
