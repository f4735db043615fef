"""Mesh extraction, host side (no GPU): the generated case table (csrc/gen_mc_table.py -> csrc/mc_table.h) against the rule it
states, meshes of the numpy reference tests/_mesh_ref.py on analytic volumes (closed, oriented, topology, enclosed volume), the
synthetic scene's teacher density, the argument checks of engine/mesh and of the C entry points, and the PLY writer."""
import ctypes as C
import itertools
import math
import os

import numpy as np
import pytest
import torch

from tests import _mesh_ref as M

GEN = M.GEN


def _crossing(case, e):
    a, b = GEN.edge_ends(e)
    return ((case >> a) & 1) != ((case >> b) & 1)


def test_generator_reproduces_the_committed_table():
    with open(os.path.join(M.CSRC, "mc_table.h")) as fh:
        assert fh.read() == GEN.header()


def test_table_sizes():
    assert max(M.NTRI) == GEN.MAX_TRIS == 5
    assert int(M.NTRI.sum()) == 820
    assert M.NTRI[0] == 0 and M.NTRI[255] == 0
    assert max(len(l) for s in range(256) for l in GEN.case_loops(s)) == 7


@pytest.mark.parametrize("case", range(256))
def test_every_case_follows_the_face_rule(case):
    tris = M.TABLE[case]
    used = {e for t in tris for e in t}
    crossing = {e for e in range(12) if _crossing(case, e)}
    assert used == crossing                                          # exactly the crossing edges, each one vertex
    # polygon boundaries: triangle sides that occur once; diagonals occur twice (fans)
    sides = {}
    for t in tris:
        for u, v in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            sides[frozenset((u, v))] = sides.get(frozenset((u, v)), 0) + 1
    boundary = {s for s, n in sides.items() if n == 1}
    diagonals = {s for s, n in sides.items() if n == 2}
    assert all(n in (1, 2) for n in sides.values())
    # every boundary side lies on a face, and per face the sides are the face rule's segments
    for f in range(6):
        rule = {frozenset((e0, e1)) for e0, e1, _ in GEN.face_segments(case, f)}
        on_f = {s for s in boundary if all(f in GEN.EDGE_FACES[e] for e in s)}
        assert on_f == rule, (case, f)
    assert sum(len(GEN.face_segments(case, f)) for f in range(6)) == len(boundary)
    # no fan diagonal joins two edges of a common face
    for s in diagonals:
        u, v = tuple(s)
        assert not (GEN.EDGE_FACES[u] & GEN.EDGE_FACES[v]), (case, u, v)


def test_neighbouring_cells_agree_on_every_shared_face():
    """The segments on face (a, 1) of a cell, in face coordinates, are those on face (a, 0) of its neighbour along a whenever the
    four shared corners agree: the boundary sides the table emits are a function of the face's corners alone."""
    def face_sides(case, a, s):
        out = set()
        for e0, e1, _ in GEN.face_segments(case, 2 * a + s):
            # an edge of the face as its two corners with bit a cleared
            out.add(frozenset(frozenset(c & ~(1 << a) for c in GEN.edge_ends(e)) for e in (e0, e1)))
        return out
    for a in range(3):
        for ca, cb in itertools.product(range(256), range(0, 256, 7)):
            top = [c for c in range(8) if (c >> a) & 1]
            if all(((ca >> c) & 1) == ((cb >> (c & ~(1 << a))) & 1) for c in top):
                assert face_sides(ca, a, 1) == face_sides(cb, a, 0)


def _grid(R, lo=-1.0, hi=1.0):
    x = (np.arange(R, dtype=np.float64) + 0.5) / R * (hi - lo) + lo
    Z, Y, X = np.meshgrid(x, x, x, indexing="ij")
    return X, Y, Z


def _check_closed(verts, faces):
    assert len(faces) > 0
    assert M.closed_and_oriented(faces)
    assert (M.undirected_edge_counts(faces) == 2).all()


def test_sphere_torus_two_spheres():
    X, Y, Z = _grid(48)
    sphere = (0.7 - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)
    v, f, n = M.marching_cubes(sphere, 0.0, [-1] * 3, [1] * 3)
    _check_closed(v, f)
    assert M.euler(v, f) == 2
    assert (np.einsum("ij,ij->i", n, v) > 0).all()                   # normals point outward: -grad of a density falling outward
    r = np.sqrt(X * X + Y * Y)
    torus = (0.22 - np.sqrt((r - 0.55) ** 2 + Z * Z)).astype(np.float32)
    v, f, n = M.marching_cubes(torus, 0.0, [-1] * 3, [1] * 3)
    _check_closed(v, f)
    assert M.euler(v, f) == 0
    two = np.maximum(0.35 - np.sqrt((X - 0.45) ** 2 + Y * Y + Z * Z), 0.35 - np.sqrt((X + 0.45) ** 2 + Y * Y + Z * Z))
    v, f, n = M.marching_cubes(two.astype(np.float32), 0.0, [-1] * 3, [1] * 3)
    _check_closed(v, f)
    assert M.euler(v, f) == 4


def test_enclosed_volume_of_a_sphere_and_a_torus():
    X, Y, Z = _grid(96)
    sphere = (0.7 - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)
    v, f, _ = M.marching_cubes(sphere, 0.0, [-1] * 3, [1] * 3)
    want = 4.0 / 3.0 * math.pi * 0.7 ** 3
    assert abs(M.enclosed_volume(v, f) / want - 1.0) < 0.01
    r = np.sqrt(X * X + Y * Y)
    torus = (0.22 - np.sqrt((r - 0.55) ** 2 + Z * Z)).astype(np.float32)
    v, f, _ = M.marching_cubes(torus, 0.0, [-1] * 3, [1] * 3)
    want = 2.0 * math.pi ** 2 * 0.55 * 0.22 ** 2
    assert abs(M.enclosed_volume(v, f) / want - 1.0) < 0.01


def test_binary_noise_volumes_are_closed_and_oriented():
    """Random inside / outside patterns reach every case and every pair of neighbouring cases: one wrong table entry breaks this."""
    seen = set()
    for seed in range(300):
        rng = np.random.default_rng(seed)
        R = int(rng.integers(4, 12))
        v = rng.random((R, R, R)).astype(np.float32)
        v[[0, -1]] = 0.0
        v[:, [0, -1]] = 0.0
        v[:, :, [0, -1]] = 0.0
        verts, faces, _ = M.marching_cubes(v, 0.5, [0.0] * 3, [1.0] * 3)
        if len(faces):
            assert M.closed_and_oriented(faces), seed
            assert M.enclosed_volume(verts, faces) > 0
        ins = (v > 0.5).astype(np.int64)
        case = sum(ins[(c >> 2):(c >> 2) + R - 1, ((c >> 1) & 1):((c >> 1) & 1) + R - 1, (c & 1):(c & 1) + R - 1] << c
                   for c in range(8))
        seen.update(np.unique(case).tolist())
    assert len(seen) == 256


def test_teacher_density_mesh_is_closed_with_the_union_volume():
    from nerf_meets_mlx_amd.dataset import synthetic
    R, lo, hi = 64, [-1.5] * 3, [1.5] * 3
    pts = torch.from_numpy(M.lattice_points(R, lo, hi))
    sigma, _ = synthetic.teacher_field(pts)
    vol = sigma.numpy().astype(np.float32).reshape(R, R, R)
    v, f, _ = M.marching_cubes(vol, 25.0, lo, hi)
    _check_closed(v, f)
    want, area = M.boxes_union([(c, h) for c, h, _ in synthetic._BOXES])
    h = 3.0 / R
    assert abs(M.enclosed_volume(v, f) - want) <= h * area, (M.enclosed_volume(v, f), want, h * area)


def test_lattice_and_gradient_arithmetic():
    R, lo, hi = 7, [-0.3, 0.1, 2.0], [0.9, 0.35, 2.7]
    h = M.spacing(R, lo, hi)
    assert h.dtype == np.float32 and h[0] == np.float32(np.float32(0.9) - np.float32(-0.3)) / np.float32(7)
    p = M.lattice_points(R, lo, hi)
    assert p.shape == (R ** 3, 3) and (p > np.float32(lo)).all() and (p < np.float32(hi)).all()
    assert p[1, 0] == np.float32(-0.3) + np.float32(1.5) * h[0] and p[R, 1] == np.float32(0.1) + np.float32(1.5) * h[1]
    lin = (np.arange(R ** 3, dtype=np.float32) * 0.25).reshape(R, R, R)         # v = 0.25 (i + R j + R^2 k)
    g = M.gradient(lin, h)
    assert np.allclose(g[..., 0], 0.25 / h[0]) and np.allclose(g[..., 1], 0.25 * R / h[1]) and np.allclose(g[..., 2], 0.25 * R * R / h[2])


def test_degenerate_volumes():
    v = np.full((5, 5, 5), 3.0, np.float32)
    for iso in (3.0, 2.0, 4.0):                                       # v == iso is outside; all inside / all outside
        verts, faces, normals = M.marching_cubes(v, iso, [0] * 3, [1] * 3)
        assert len(verts) == 0 and len(faces) == 0
    v[2, 2, 2] = np.nan                                               # NaN is outside
    verts, faces, normals = M.marching_cubes(v, 2.0, [0] * 3, [1] * 3)
    assert len(verts) == 6 and len(faces) > 0 and M.closed_and_oriented(faces)
    # t = NaN -> 0.5: every vertex is the midpoint of an edge of the NaN point, h / 2 = 0.1 from it along one axis
    mids = (np.array([2.0, 2.0, 2.0]) + 0.5) / 5
    assert np.allclose(np.sort(np.abs(verts - mids).max(1)), 0.1, atol=1e-6)
    assert (normals == 0).all()                                       # the gradient is NaN around the NaN


# ------------------------------------------------------------------------------------------------ argument checks
def test_check_mesh_args():
    from nerf_meets_mlx_amd.engine.mesh import check_mesh_args
    assert check_mesh_args(2, [0, 0, 0], [1, 1, 1], 0) == (2, [0.0] * 3, [1.0] * 3, 0.0)
    assert check_mesh_args(512, [-1.5] * 3, [1.5] * 3, 2.5)[0] == 512
    for bad in (1, 513, 0, -4, 2.0, True, "64", None):
        with pytest.raises(ValueError):
            check_mesh_args(bad, [0] * 3, [1] * 3, 0)
    for lo, hi in (([0, 0, 1], [1, 1, 1]), ([0, 0, 2], [1, 1, 1]), ([0, 0, float("nan")], [1, 1, 1]),
                   ([0, 0, 0], [1, 1, float("inf")]), ([0, 0], [1, 1])):
        with pytest.raises(ValueError):
            check_mesh_args(8, lo, hi, 0)
    for iso in (float("nan"), float("inf"), -float("inf"), None, "1"):
        with pytest.raises(ValueError):
            check_mesh_args(8, [0] * 3, [1] * 3, iso)


def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    lo, hi = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    bad_hi = (C.c_float * 3)(1, 0, 1)
    nan_hi = (C.c_float * 3)(1, 1, float("nan"))
    fake = C.c_void_p(0x1000)                                          # never dereferenced: every call below fails its checks first
    E_NULL, E_SHAPE = -1, -2
    assert L.nerf_mesh_workspace_bytes(1) == -1 and L.nerf_mesh_workspace_bytes(513) == -1
    assert L.nerf_mesh_workspace_bytes(2) == 2 * 8 + 8 * 4
    assert L.nerf_mesh_workspace_bytes(512) == 2 * 8 * (512 ** 3 // 256) + 4 * 512 ** 3
    # points
    assert L.nerf_mesh_points(1, lo, hi, 0, 1, fake, fake, None) == E_SHAPE
    assert L.nerf_mesh_points(513, lo, hi, 0, 1, fake, fake, None) == E_SHAPE
    assert L.nerf_mesh_points(4, None, hi, 0, 1, fake, fake, None) == E_NULL
    assert L.nerf_mesh_points(4, lo, bad_hi, 0, 1, fake, fake, None) == E_SHAPE
    assert L.nerf_mesh_points(4, lo, nan_hi, 0, 1, fake, fake, None) == E_SHAPE
    assert L.nerf_mesh_points(4, lo, hi, 60, 5, fake, fake, None) == E_SHAPE
    assert L.nerf_mesh_points(4, lo, hi, -1, 1, fake, fake, None) == E_SHAPE
    assert L.nerf_mesh_points(4, lo, hi, 0, 1, None, fake, None) == E_NULL
    assert L.nerf_mesh_points(4, lo, hi, 64, 0, None, None, None) == 0          # nothing to do
    # count
    assert L.nerf_mesh_count(fake, 1, 0.0, fake, fake, None) == E_SHAPE
    assert L.nerf_mesh_count(fake, 8, float("nan"), fake, fake, None) == E_SHAPE
    assert L.nerf_mesh_count(fake, 8, float("inf"), fake, fake, None) == E_SHAPE
    assert L.nerf_mesh_count(None, 8, 0.0, fake, fake, None) == E_NULL
    assert L.nerf_mesh_count(fake, 8, 0.0, None, fake, None) == E_NULL
    assert L.nerf_mesh_count(fake, 8, 0.0, fake, None, None) == E_NULL
    # vertices
    assert L.nerf_mesh_write_vertices(fake, 600, 0.0, lo, hi, fake, 1, fake, fake, None, None) == E_SHAPE
    assert L.nerf_mesh_write_vertices(fake, 8, 0.0, lo, bad_hi, fake, 1, fake, fake, None, None) == E_SHAPE
    assert L.nerf_mesh_write_vertices(fake, 8, 0.0, None, hi, fake, 1, fake, fake, None, None) == E_NULL
    assert L.nerf_mesh_write_vertices(fake, 8, 0.0, lo, hi, fake, 3 * 512 + 1, fake, fake, None, None) == E_SHAPE
    assert L.nerf_mesh_write_vertices(fake, 8, 0.0, lo, hi, fake, -1, fake, fake, None, None) == E_SHAPE
    assert L.nerf_mesh_write_vertices(fake, 8, 0.0, lo, hi, fake, 5, fake, None, None, None) == E_NULL
    assert L.nerf_mesh_write_vertices(None, 8, 0.0, lo, hi, fake, 5, fake, fake, None, None) == E_NULL
    assert L.nerf_mesh_write_vertices(None, 8, 0.0, lo, hi, None, 0, None, None, None, None) == 0     # V = 0: no launch
    # faces
    assert L.nerf_mesh_write_faces(fake, 8, float("nan"), fake, 1, fake, None) == E_SHAPE
    assert L.nerf_mesh_write_faces(fake, 8, 0.0, fake, 5 * 512 + 1, fake, None) == E_SHAPE
    assert L.nerf_mesh_write_faces(fake, 8, 0.0, fake, 1, None, None) == E_NULL
    assert L.nerf_mesh_write_faces(None, 8, 0.0, None, 0, None, None) == 0                            # F = 0: no launch


def test_write_ply_round_trip(tmp_path):
    from nerf_meets_mlx_amd.engine.mesh import Mesh, read_ply, write_ply
    X, Y, Z = _grid(12)
    v, f, n = M.marching_cubes((0.6 - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32), 0.0, [-1] * 3, [1] * 3)
    rng = np.random.default_rng(0)
    col = rng.random((len(v), 3)).astype(np.float32)
    col[0] = [0.0, 1.0, 0.5]
    for colors in (None, torch.from_numpy(col)):
        mesh = Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n), colors)
        p = write_ply(str(tmp_path / "m.ply"), mesh)
        assert not os.path.exists(p + ".tmp")
        raw = open(p, "rb").read()
        head = raw[:raw.index(b"end_header\n")].decode().splitlines()
        assert head[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
        assert f"element face {len(f)}" in head and "property list uchar int vertex_indices" in head
        assert ("property uchar red" in head) == (colors is not None)
        back = read_ply(p)
        assert np.array_equal(back.verts.numpy(), v) and np.array_equal(back.normals.numpy(), n)
        assert np.array_equal(back.faces.numpy(), f)
        if colors is None:
            assert back.colors is None
        else:
            want = np.round(255.0 * col.astype(np.float64)).astype(np.uint8)
            assert np.array_equal(np.round(back.colors.numpy() * 255.0).astype(np.uint8), want)
            assert tuple(np.round(back.colors.numpy()[0] * 255).astype(int)) == (0, 255, 128)
        # vertex block: 24 or 27 bytes per vertex; faces 13 bytes each
        body = len(raw) - (raw.index(b"end_header\n") + len(b"end_header\n"))
        assert body == len(v) * (27 if colors is not None else 24) + 13 * len(f)
