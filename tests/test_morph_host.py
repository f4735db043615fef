"""Morphological opening, host side (no GPU): the properties include/nerf_hip.h "morphological opening" states, checked on the
reference tests/_morph_ref.py at R <= 17 (the erosion against the direct ball definition, the reconstruction between the
classical opening and M, idempotence, the dumbbell's numbers, the C-channel, the weaker sub-mesh property through the marching
cubes of tests/_mesh_ref.py), the argument checks of engine/mesh/volume.py and of the C entry points, and the exported symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _ccl_ref as CC
from tests import _mesh_ref as M
from tests import _morph_ref as MR

CASES = [(R, r, q) for R in (2, 3, 9, 17) for r in (1, 2, 3) for q in (0.3, 0.5, 0.7)]


def _noise_case(R, q):
    v = MR.smoothed_noise(R, 40 + R)
    return v, float(np.quantile(v, q))


@pytest.mark.parametrize("R,r,q", CASES)
def test_erosion_is_the_direct_ball_definition(R, r, q):
    v, iso = _noise_case(R, q)
    m = CC.inside_mask(v, iso)
    e = MR.erode_mask(m, r)
    assert np.array_equal(e, MR.erode_direct(m, r))
    core, stats = MR.erode(v, iso, r)
    assert np.array_equal(CC.inside_mask(core, iso), e) and stats.tolist() == [int(m.sum()), int(e.sum())]
    changed = core.view(np.uint32) != v.view(np.uint32)
    assert np.array_equal(changed, m & ~e) and (core[changed] == np.float32(iso)).all()


def test_the_box_faces_erode_and_the_l1_ball_rounds_the_box():
    R = 9
    v = np.full((R, R, R), 2.0, np.float32)
    face = np.minimum(np.arange(R), R - 1 - np.arange(R))            # distance to the nearer face along one axis
    for r in (1, 2, 4, 5):
        e = CC.inside_mask(MR.erode(v, 1.0, r)[0], 1.0)
        want = np.zeros_like(e)
        if R - 2 * r > 0:                                            # the voxels >= r from every face
            want[r:R - r, r:R - r, r:R - r] = True
        assert np.array_equal(e, want)
        # r steps of the 6-neighbour ball from that inner box reach a voxel exactly when its shortfalls to the inner box add up
        # to at most r: the faces come back, the edges and corners of the box (shortfall 2 r and 3 r) do not
        short = np.maximum(0, r - face)
        back = (short[:, None, None] + short[None, :, None] + short[None, None, :] <= r) & want.any()
        d = CC.inside_mask(MR.open_components(v, 1.0, r), 1.0)
        assert np.array_equal(d, back) and not d[0, 0, 0] and (not want.any() or d[0, R // 2, R // 2])


@pytest.mark.parametrize("R,r,q", CASES)
def test_reconstruction_lies_between_the_classical_opening_and_m_and_is_idempotent(R, r, q):
    v, iso = _noise_case(R, q)
    m = CC.inside_mask(v, iso)
    e = MR.erode_mask(m, r)
    out = MR.open_components(v, iso, r)
    d = CC.inside_mask(out, iso)
    assert (MR.dilate_ball(e, r) <= d).all() and (d <= m).all()
    assert np.array_equal(MR.erode_mask(d, r), e)                     # the core of the result is the core
    again = MR.open_components(out, iso, r)
    assert np.array_equal(again.view(np.uint32), out.view(np.uint32))
    # with a filter in between: still inside M, still at least the kept core's classical dilation
    core = MR.erode(v, iso, r)[0]
    kept = CC.inside_mask(CC.filter_volume(core, iso, 0, True), iso)
    d1 = CC.inside_mask(MR.open_components(v, iso, r, 0, True), iso)
    assert (MR.dilate_ball(kept, r) & m >= d1).all() and (d1 <= d).all() and (kept <= d1).all()


def test_values_move_as_bits_and_seeds_outside_m_are_ignored():
    v, iso = _noise_case(9, 0.5)
    v = v.copy()
    v.reshape(-1).view(np.uint32)[3] = 0x7FC12345                    # a NaN with a payload: outside
    v[4, 4, 4] = iso                                                 # exactly iso: outside
    m = CC.inside_mask(v, iso)
    assert not m.reshape(-1)[3] and not m[4, 4, 4]
    for fn in (lambda: MR.erode(v, iso, 1)[0], lambda: MR.open_components(v, iso, 1)):
        assert fn().reshape(-1).view(np.uint32)[3] == 0x7FC12345
    kept = np.full_like(v, iso + 1.0)                                # seeds everywhere, also outside M
    out, stats = MR.reconstruct(v, kept, iso, 1)
    assert np.array_equal(out.view(np.uint32), v.view(np.uint32)) and stats.tolist() == [int(m.sum()), int(m.sum())]
    out, stats = MR.reconstruct(v, np.full_like(v, iso), iso, 3)      # no seeds: everything is dropped
    assert not CC.inside_mask(out, iso).any() and stats.tolist() == [0, 0]


def test_dumbbell_numbers():
    v, bridge, cube = MR.dumbbell()
    iso, r = 0.5, 1
    assert v.shape == (17, 17, 17) and int(bridge.sum()) == 5
    assert CC.components(v, iso)[2].tolist()[:2] == [1, 7 ** 3 + 5 ** 3 + 5]         # one component: the filter alone keeps all
    core, stats = MR.erode(v, iso, r)
    e = CC.inside_mask(core, iso)
    assert stats.tolist() == [473, 152] and 152 == 5 ** 3 + 3 ** 3
    want = np.zeros_like(e)
    want[2:7, 2:7, 1:6] = True                                       # the cubes' cores, nothing of the bridge
    want[2:5, 2:5, 13:16] = True
    assert np.array_equal(e, want) and CC.components(core, iso)[2].tolist()[:2] == [2, 152]
    d = CC.inside_mask(MR.open_components(v, iso, r, 0, True), iso)
    assert not (d & ~cube & ~bridge).any() and int((d & bridge).sum()) <= r          # the big cube + at most r of the stump
    assert (MR.dilate_ball(want & cube, r) <= d).all() and int(d.sum()) == 5 ** 3 + 6 * 25
    # the plain opening (no filter) keeps both cubes and cuts the bridge's middle
    d0 = CC.inside_mask(MR.open_components(v, iso, r), iso)
    assert int((d0 & bridge).sum()) <= 2 * r and (d0 & ~cube & ~bridge).any()
    # a bar on the faces' centres leaves the two face voxels it touches in the core
    assert MR.erode(MR.dumbbell(at=2)[0], iso, r)[1].tolist() == [473, 154]


@pytest.mark.parametrize("r", [2, 3])
def test_reconstruction_does_not_jump_a_gap(r):
    v, seeds, upper = MR.c_channel(17, gap=1)
    iso = 0.5
    m = CC.inside_mask(v, iso)
    kept = np.where(seeds, v, np.float32(0.0)).astype(np.float32)
    d = CC.inside_mask(MR.reconstruct(v, kept, iso, r)[0], iso)
    assert (MR.dilate_ball(seeds, r) & m & upper).any()              # plain dilate-and-mask reaches the other arm
    assert not (d & upper).any() and (seeds <= d).all()


@pytest.mark.parametrize("kw", [dict(), dict(largest_only=True), dict(min_component=20)])
def test_weaker_sub_mesh_property_on_the_cpu(kw):
    R, r, lo, hi = 17, 1, [-1.0] * 3, [1.0] * 3
    v = MR.smoothed_noise(R, 5)
    iso = float(np.quantile(v, 0.6))
    out = MR.open_components(v, iso, r, **kw)
    d, m = CC.inside_mask(out, iso), CC.inside_mask(v, iso)
    assert d.any() and (m & ~d).any()
    v0, _, _ = M.marching_cubes(v, iso, lo, hi)
    v1, f1, _ = M.marching_cubes(out, iso, lo, hi)
    in_out, in_vol = MR.original_edge_masks(v, out, iso)
    assert len(in_out) == len(v1) and len(in_vol) == len(v0) and 0 < in_out.sum() == in_vol.sum()
    assert np.array_equal(v1[in_out].view(np.uint32), v0[in_vol].view(np.uint32))    # bit for bit and in order
    # the other vertices are cuts: the edge's outside end is a dropped voxel (value iso exactly), the vertex sits on it
    cross, low = MR.crossing_edges(out, iso)
    own = np.argwhere(cross)[~in_out]                                 # [n, 4] = (k, j, i, axis)
    assert len(own) == int((~in_out).sum()) > 0
    step = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]])
    pts = M.axis_coords(R, lo, hi)
    for (k, j, i, a), x in zip(own.tolist(), v1[~in_out]):
        q = np.array([k, j, i])
        cut = q + step[a] if low[k, j, i, a] else q
        assert (m & ~d)[tuple(cut)] and out[tuple(cut)] == np.float32(iso)
        assert np.allclose(x, [pts[0][cut[2]], pts[1][cut[1]], pts[2][cut[0]]], rtol=0, atol=1e-6)
    assert len(f1) > 0


def test_a_thin_field_has_an_empty_core_and_an_empty_mesh():
    R = 9
    v = np.zeros((R, R, R), np.float32)
    v[3:5, :, :] = 1.0                                               # a slab 2 voxels thick: thinner than 2 r + 1
    out = MR.open_components(v, 0.5, 1, 0, True)
    assert not CC.inside_mask(out, 0.5).any()
    verts, faces, _ = M.marching_cubes(out, 0.5, [0.0] * 3, [1.0] * 3)
    assert len(verts) == 0 and len(faces) == 0


# ------------------------------------------------------------------------------------------------ public interface
def test_check_opening_args():
    from nerf_meets_mlx_amd.engine import mesh
    assert mesh.MAX_OPENING_RADIUS == 16 == MR.MAX_RADIUS
    assert mesh.check_opening_args(0) == 0 and mesh.check_opening_args(16) == 16 and mesh.check_opening_args(np.int64(3)) == 3
    for bad in (True, False, 1.0, 2.5, -1, 17, "3", None):
        with pytest.raises(ValueError):
            mesh.check_opening_args(bad)


def test_python_entries_refuse_bad_arguments_without_a_device():
    from nerf_meets_mlx_amd.engine import mesh
    vol = torch.zeros(4, 4, 4)
    for bad in (torch.zeros(4, 4, 5), torch.zeros(4, 4), torch.zeros(4, 4, 4, dtype=torch.float64), torch.zeros(4, 4, 8)[:, :, ::2],
                np.zeros((4, 4, 4), np.float32), torch.zeros(1, 1, 1)):
        with pytest.raises(ValueError):
            mesh.erode(bad, 0.0, 1)
        with pytest.raises(ValueError):
            mesh.reconstruct(bad, bad, 0.0, 1)
        with pytest.raises(ValueError):
            mesh.reconstruct(vol, bad, 0.0, 1)                        # kept must match the volume
        with pytest.raises(ValueError):
            mesh.open_components(bad, 0.0, 1)
    for iso in (float("nan"), float("inf"), None):
        with pytest.raises(ValueError):
            mesh.erode(vol, iso, 1)
    for radius in (0, 17, -1, True, 1.0, None):
        with pytest.raises(ValueError):
            mesh.erode(vol, 0.0, radius)
        with pytest.raises(ValueError):
            mesh.reconstruct(vol, vol, 0.0, radius)
        with pytest.raises(ValueError):
            mesh.open_components(vol, 0.0, radius)
    for kw in (dict(min_component=-1), dict(min_component=65), dict(largest_only=1)):
        with pytest.raises(ValueError):
            mesh.open_components(vol, 0.0, 1, **kw)

    def query(rays, z):
        raise AssertionError("the field is queried only after the argument checks")
    for bad in (-1, 17, True, 1.0, "1", None):
        with pytest.raises(ValueError):
            mesh.extract(query, mesh.RELU, 4, 0.0, [0] * 3, [1] * 3, device="cpu", opening_radius=bad)


def test_trainer_extract_mesh_checks_the_opening_radius_before_the_field():
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    from nerf_meets_mlx_amd.engine.trainer import Trainer

    class Stub(Trainer):
        def __init__(self):
            pass

        def _mesh_field(self):
            raise AssertionError("the field is touched only after the argument checks")

    box = ([0.0] * 3, [1.0] * 3)
    for bad in (-1, 17, True, 2.0, "2", None):
        with pytest.raises(ValueError):
            Stub().extract_mesh(8, 0.5, box, opening_radius=bad)
    with pytest.raises(AssertionError):                              # valid arguments reach the field
        Stub().extract_mesh(8, 0.5, box, largest_only=True, opening_radius=16)
    assert NGPTrainer.extract_mesh is Trainer.extract_mesh


def test_library_exports_the_entry_points_and_the_header_declares_them():
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    names = ("nerf_morph_workspace_bytes", "nerf_morph_erode", "nerf_morph_reconstruct")
    with open(os.path.join(M.ROOT, "include", "nerf_hip.h")) as fh:
        header = fh.read()
    for name in names:
        assert hasattr(L, name) and name in N.SIGNATURES
        assert re.search(r"\b" + name + r"\(", header)
    assert "morphological opening" in header and re.search(r"#define\s+NERF_MORPH_MAX_RADIUS\s+16\b", header)
    assert header.index("connected components") < header.index("morphological opening") and L.nerf_abi_version() == 3


def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    fake = C.c_void_p(0x1000)                                          # never dereferenced: every call below fails its checks first
    E_NULL, E_SHAPE = -1, -2
    assert L.nerf_morph_workspace_bytes(1) == -1 and L.nerf_morph_workspace_bytes(513) == -1
    assert L.nerf_morph_workspace_bytes(0) == -1 and L.nerf_morph_workspace_bytes(-5) == -1
    for R in (2, 63, 64, 65, 128, 512):                              # three masks of ceil(R / 64) 64-bit words per row
        assert L.nerf_morph_workspace_bytes(R) == 3 * 8 * ((R + 63) // 64) * R * R
    erode = lambda R=8, iso=0.0, r=1, p=(fake,) * 4: L.nerf_morph_erode(p[0], R, iso, r, p[1], p[2], p[3], None)
    recon = lambda R=8, iso=0.0, r=1, p=(fake,) * 5: L.nerf_morph_reconstruct(p[0], p[1], R, iso, r, p[2], p[3], p[4], None)
    assert erode(r=16, p=(None,) + (fake,) * 3) == E_NULL            # valid values reach the pointer check
    for R in (1, 513, 0, -3):
        assert erode(R=R) == E_SHAPE and recon(R=R) == E_SHAPE
    for iso in (float("nan"), float("inf"), float("-inf")):
        assert erode(iso=iso) == E_SHAPE and recon(iso=iso) == E_SHAPE
    for r in (0, 17, -1, 1 << 20):
        assert erode(r=r) == E_SHAPE and recon(r=r) == E_SHAPE
    for k in range(4):
        p = [fake] * 4
        p[k] = None
        assert erode(p=p) == E_NULL
    for k in range(5):
        p = [fake] * 5
        p[k] = None
        assert recon(p=p) == E_NULL
