"""Connected components, host side (no GPU): the reference tests/_ccl_ref.py against first principles (a breadth-first search
written out here) on small volumes, the sub-mesh property of include/nerf_hip.h "connected components" through the marching
cubes of tests/_mesh_ref.py, the argument checks of engine/mesh/volume.py and of the C entry points, and the exported symbols."""
import ctypes as C
import os
import re
from collections import deque

import numpy as np
import pytest
import torch

from tests import _ccl_ref as CC
from tests import _mesh_ref as M


def _bfs_components(ins):
    """[set of linear indices] of the 6-connected components of a bool [R, R, R] mask, by breadth-first search."""
    R = ins.shape[0]
    seen = np.zeros_like(ins)
    comps = []
    for k0, j0, i0 in zip(*np.nonzero(ins)):
        if seen[k0, j0, i0]:
            continue
        seen[k0, j0, i0] = True
        todo, comp = deque([(int(k0), int(j0), int(i0))]), set()
        while todo:
            k, j, i = todo.popleft()
            comp.add(i + R * (j + R * k))
            for dk, dj, di in ((0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)):
                a, b, c = k + dk, j + dj, i + di
                if 0 <= a < R and 0 <= b < R and 0 <= c < R and ins[a, b, c] and not seen[a, b, c]:
                    seen[a, b, c] = True
                    todo.append((a, b, c))
        comps.append(comp)
    return comps


def _noise(R, seed):
    return np.random.default_rng(seed).standard_normal((R, R, R)).astype(np.float32)


@pytest.mark.parametrize("R,iso,seed", [(2, 0.0, 0), (3, 0.0, 1), (5, 0.0, 2), (7, 0.6, 3), (9, -0.3, 4)])
def test_reference_labels_sizes_and_stats_from_first_principles(R, iso, seed):
    v = _noise(R, seed)
    v.reshape(-1)[::11] = np.nan                                     # NaN and exact-iso voxels are outside
    v.reshape(-1)[5::13] = iso
    ins = CC.inside_mask(v, iso)
    assert not ins.reshape(-1)[::11].any() and not ins.reshape(-1)[5::13].any()
    labels, sizes, stats = CC.components(v, iso)
    comps = _bfs_components(ins)
    flat = ins.reshape(-1)
    assert labels.dtype == np.int32 and sizes.dtype == np.int32 and stats.dtype == np.int64
    assert (labels[~flat] == -1).all()
    covered = set()
    for comp in comps:
        idx = sorted(comp)
        assert (labels[idx] == idx[0]).all()                         # the component's minimum
        assert sizes[idx[0]] == len(idx) and (sizes[idx[1:]] == 0).all()
        assert not (covered & comp)                                  # a partition of the inside set
        covered |= comp
    assert covered == set(np.flatnonzero(flat).tolist())
    assert int(sizes.sum()) == int(flat.sum()) and (sizes[~flat] == 0).all()
    best = max(comps, key=lambda c: (len(c), -min(c))) if comps else None
    assert stats.tolist() == [len(comps), int(flat.sum()), min(best) if best else -1]


def test_reference_neighbourhood_is_the_six_faces_without_wrap():
    R = 4
    v = np.zeros((R, R, R), np.float32)
    v[0, 0, R - 1] = v[0, 1, 0] = 1.0                                # adjacent in memory, not neighbours
    v[2, 2, 2] = v[3, 3, 3] = v[2, 3, 3] = 1.0                       # a body diagonal (apart) and a face neighbour (joined)
    v[0, 2, 2] = v[0, 3, 3] = 1.0                                    # a face diagonal (apart)
    labels, sizes, stats = CC.components(v, 0.5)
    lin = lambda k, j, i: i + R * (j + R * k)
    assert labels[lin(0, 0, R - 1)] == lin(0, 0, R - 1) and labels[lin(0, 1, 0)] == lin(0, 1, 0)
    assert labels[lin(2, 2, 2)] == lin(2, 2, 2)
    assert labels[lin(3, 3, 3)] == labels[lin(2, 3, 3)] == lin(2, 3, 3)
    assert labels[lin(0, 2, 2)] != labels[lin(0, 3, 3)]
    assert stats.tolist() == [6, 7, lin(2, 3, 3)]


def _two_cubes(R=8, n=2):
    v = np.zeros((R, R, R), np.float32)
    v[1:1 + n, 1:1 + n, 1:1 + n] = 2.0
    v[5:5 + n, 4:4 + n, 3:3 + n] = 3.0
    v[0, 7, 7] = 1.0                                                 # a speck
    return v


def test_reference_filter_edge_values_and_tie_break():
    v = _two_cubes()
    iso = 0.5
    labels, sizes, stats = CC.components(v, iso)
    R = 8
    first, second, speck = 1 + R * (1 + R * 1), 3 + R * (4 + R * 5), 7 + R * (7 + R * 0)
    assert stats.tolist() == [3, 17, first]                          # two components of 8: the smaller label is the largest
    assert sizes[first] == 8 and sizes[second] == 8 and sizes[speck] == 1
    for m in (0, 1):
        assert np.array_equal(CC.filter_volume(v, iso, m).view(np.uint32), v.view(np.uint32))
    out = CC.filter_volume(v, iso, 2)
    assert out[0, 7, 7] == np.float32(iso) and (out[v > 1.5] == v[v > 1.5]).all()
    assert np.array_equal(CC.filter_volume(v, iso, 8), out)          # size: kept
    assert (CC.filter_volume(v, iso, 9) == np.where(v > iso, np.float32(iso), v)).all()      # size + 1: nothing survives
    only = CC.filter_volume(v, iso, 0, largest_only=True)
    assert (only[1:3, 1:3, 1:3] == 2.0).all() and (only[5:7, 4:6, 3:5] == np.float32(iso)).all() and only[0, 7, 7] == np.float32(iso)
    assert not CC.inside_mask(CC.filter_volume(v, iso, 9, largest_only=True), iso).any()
    # kept and outside values move as bits
    w = v.copy()
    w.reshape(-1).view(np.uint32)[0] = 0x7FC12345                    # a NaN with a payload, outside
    assert CC.filter_volume(w, iso, 2).reshape(-1).view(np.uint32)[0] == 0x7FC12345


def _two_noisy_blobs(R=17, seed=0):
    rng = np.random.default_rng(seed)
    x = (np.arange(R) + 0.5) / R * 2 - 1
    Z, Y, X = np.meshgrid(x, x, x, indexing="ij")
    big = 0.55 - np.sqrt((X + 0.3) ** 2 + Y * Y + Z * Z)
    small = 0.25 - np.sqrt((X - 0.6) ** 2 + (Y - 0.5) ** 2 + (Z + 0.4) ** 2)
    return (np.maximum(big, small) + 0.08 * rng.standard_normal((R, R, R))).astype(np.float32)


@pytest.mark.parametrize("kw", [dict(min_voxels=0, largest_only=True), dict(min_voxels=6), dict(min_voxels=40, largest_only=True)])
def test_sub_mesh_property_on_the_cpu(kw):
    v, iso, lo, hi = _two_noisy_blobs(), 0.0, [-1.0] * 3, [1.0] * 3
    comps = CC.components(v, iso)
    assert comps[2][0] > 2                                           # the blobs and specks
    f = CC.filter_volume(v, iso, comps=comps, **kw)
    drop = CC.dropped_mask(*comps, **kw)
    assert drop.any() and not drop[comps[0] >= 0].all()
    v0, f0, _ = M.marching_cubes(v, iso, lo, hi)
    v1, f1, _ = M.marching_cubes(f, iso, lo, hi)
    keep = CC.kept_vertex_mask(v, iso, drop)
    assert len(keep) == len(v0) and 0 < keep.sum() < len(v0)
    assert v1.shape == v0[keep].shape and np.array_equal(v1.view(np.uint32), v0[keep].view(np.uint32))
    assert len(f1) > 0 and M.closed_and_oriented(f1)
    # no lattice edge joins a dropped voxel to a kept inside voxel
    ins = CC.inside_mask(f, iso).reshape(-1)
    e = CC.inside_edges(CC.inside_mask(v, iso))
    assert (drop[e[:, 0]] == drop[e[:, 1]]).all() and not ins[drop].any()


# ------------------------------------------------------------------------------------------------ public interface
def test_check_component_args():
    from nerf_meets_mlx_amd.engine.mesh import check_component_args
    assert check_component_args(0, False, 8) == (0, False)
    assert check_component_args(512, True, 8) == (512, True)
    assert check_component_args(np.int64(7), False, 8) == (7, False)
    for bad in (True, False, 1.0, 2.5, -1, 513, "3", None):
        with pytest.raises(ValueError):
            check_component_args(bad, False, 8)
    for bad in (0, 1, None, "yes", np.bool_(True)):
        with pytest.raises(ValueError):
            check_component_args(0, bad, 8)


def test_python_entries_refuse_bad_arguments_without_a_device():
    from nerf_meets_mlx_amd.engine import mesh
    vol = torch.zeros(4, 4, 4)
    for bad in (torch.zeros(4, 4, 5), torch.zeros(4, 4), torch.zeros(4, 4, 4, dtype=torch.float64), torch.zeros(4, 4, 8)[:, :, ::2],
                np.zeros((4, 4, 4), np.float32), torch.zeros(1, 1, 1)):
        with pytest.raises(ValueError):
            mesh.connected_components(bad, 0.0)
        with pytest.raises(ValueError):
            mesh.filter_components(bad, 0.0)
    for iso in (float("nan"), float("inf"), None):
        with pytest.raises(ValueError):
            mesh.connected_components(vol, iso)
    for kw in (dict(min_component=-1), dict(min_component=65), dict(min_component=True), dict(min_component=2.0),
               dict(largest_only=1), dict(largest_only=None)):
        with pytest.raises(ValueError):
            mesh.filter_components(vol, 0.0, **kw)

        def query(rays, z):
            raise AssertionError("the field is queried only after the argument checks")
        with pytest.raises(ValueError):
            mesh.extract(query, mesh.RELU, 4, 0.0, [0] * 3, [1] * 3, device="cpu", **kw)


def test_trainer_extract_mesh_checks_its_arguments_before_the_field():
    from nerf_meets_mlx_amd.engine.trainer import Trainer

    class Stub(Trainer):
        def __init__(self):
            pass

        def _mesh_field(self):
            raise AssertionError("the field is touched only after the argument checks")

    box = ([0.0] * 3, [1.0] * 3)
    for kw in (dict(min_component=-1), dict(min_component=8 ** 3 + 1), dict(min_component=False), dict(min_component=1.5),
               dict(largest_only=1), dict(largest_only="no")):
        with pytest.raises(ValueError):
            Stub().extract_mesh(8, 0.5, box, **kw)
    with pytest.raises(AssertionError):                              # valid arguments reach the field
        Stub().extract_mesh(8, 0.5, box, min_component=8 ** 3, largest_only=True)


def test_library_exports_the_entry_points_and_the_header_declares_them():
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    names = ("nerf_ccl_workspace_bytes", "nerf_ccl_label", "nerf_ccl_sizes", "nerf_ccl_filter")
    with open(os.path.join(M.ROOT, "include", "nerf_hip.h")) as fh:
        header = fh.read()
    for name in names:
        assert hasattr(L, name)
        assert re.search(r"\b" + name + r"\(", header)
    assert "connected components" in header and L.nerf_abi_version() == 3


def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    fake = C.c_void_p(0x1000)                                          # never dereferenced: every call below fails its checks first
    E_NULL, E_SHAPE = -1, -2
    assert L.nerf_ccl_workspace_bytes(1) == -1 and L.nerf_ccl_workspace_bytes(513) == -1
    assert L.nerf_ccl_workspace_bytes(2) == 4 * 8 and L.nerf_ccl_workspace_bytes(512) == 4 * 512 ** 3
    for R in (1, 513, 0, -3):
        assert L.nerf_ccl_label(fake, R, 0.0, fake, fake, None) == E_SHAPE
        assert L.nerf_ccl_sizes(fake, R, fake, fake, None) == E_SHAPE
        assert L.nerf_ccl_filter(fake, fake, fake, fake, R, 0.0, 0, 0, fake, None) == E_SHAPE
    for iso in (float("nan"), float("inf")):
        assert L.nerf_ccl_label(fake, 8, iso, fake, fake, None) == E_SHAPE
        assert L.nerf_ccl_filter(fake, fake, fake, fake, 8, iso, 0, 0, fake, None) == E_SHAPE
    assert L.nerf_ccl_filter(fake, fake, fake, fake, 8, 0.0, -1, 0, fake, None) == E_SHAPE
    for k in range(3):
        a = [fake, fake, fake]
        a[k] = None
        assert L.nerf_ccl_label(a[0], 8, 0.0, a[1], a[2], None) == E_NULL
        assert L.nerf_ccl_sizes(a[0], 8, a[1], a[2], None) == E_NULL
    for k in range(5):
        a = [fake] * 5
        a[k] = None
        assert L.nerf_ccl_filter(a[0], a[1], a[2], a[3], 8, 0.0, 0, 0, a[4], None) == E_NULL
