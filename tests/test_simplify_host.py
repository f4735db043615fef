"""Mesh simplification without a GPU: properties of the numpy reference (tests/_simplify_ref.py) of include/nerf_hip.h "mesh
simplification" on marching-cubes meshes at R = 32 in [-1, 1]^3, the argument checks of engine.mesh, and the header / binding
bookkeeping.  The GPU side is held to this reference bit for bit in tests/test_gpu_simplify.py."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _mesh_ref as M
from tests import _simplify_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _simplify(name, G, placement="quadric", colors=False):
    (v, f, n, c), info = S.expected(name, G, placement, colors)
    return v, f, n, c, info


def _opposite_pairs(faces):
    """Vertex sets that carry surviving faces of both orientations."""
    f = np.asarray(faces, np.int64)
    if len(f) == 0:
        return 0
    s = np.sort(f, 1)
    m = int(f.max()) + 1
    key = (s[:, 0] * m + s[:, 1]) * m + s[:, 2]
    odd = ((f[:, 0] < f[:, 1]).astype(int) + (f[:, 1] < f[:, 2]) + (f[:, 0] < f[:, 2])) & 1
    return len(np.intersect1d(key[odd == 0], key[odd == 1]))


@pytest.mark.parametrize("G,sizes", [(4, (28, 52)), (8, (99, 194)), (12, (200, 396))])
def test_sphere_stays_closed_and_oriented(G, sizes):
    v_in, f_in, _, _ = S.mesh("sphere")
    assert (len(v_in), len(f_in)) == (1732, 3460) and M.closed_and_oriented(f_in)
    for placement in ("quadric", "mean"):
        v, f, n, _, info = _simplify("sphere", G, placement)
        assert (len(v), len(f)) == sizes
        assert M.closed_and_oriented(f)
        assert len(n) == len(v) and np.allclose(np.linalg.norm(n.astype(np.float64), axis=1), 1.0, atol=1e-6)
        assert M.enclosed_volume(v, f) > 0                           # still outward
    if G == 8:                                                       # the second compaction has work: a cluster nobody uses
        assert info["K"] == 101 and len(v) == 99


@pytest.mark.parametrize("G", S.GRIDS)
def test_quadric_placement_keeps_the_box_better_than_the_mean(G):
    vq = _simplify("box", G, "quadric")[0]
    vm = _simplify("box", G, "mean")[0]
    (cq, sq), (cm, sm) = S.box_errors(vq), S.box_errors(vm)
    assert cq < cm, (cq, cm)
    assert sq < sm, (sq, sm)
    assert len(vq) == len(vm) and np.array_equal(_simplify("box", G, "quadric")[1], _simplify("box", G, "mean")[1])


@pytest.mark.parametrize("G", S.GRIDS)
def test_plate_annihilates(G):
    v_in, f_in, _, _ = S.mesh("plate")
    assert (len(v_in), len(f_in)) == (880, 1756)
    v, f, n, c, info = _simplify("plate", G, "quadric", True)
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3) and c.shape == (0, 3)
    assert info["K"] > 0 and not info["keep"].any()


@pytest.mark.parametrize("G", S.GRIDS)
def test_noise_volume_has_no_degenerate_face_isolated_vertex_or_opposite_pair(G):
    v, f, _, _, _ = _simplify("noise", G)
    assert len(f) > 0
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all()
    assert np.array_equal(np.unique(f), np.arange(len(v)))
    assert _opposite_pairs(f) == 0


def test_a_fine_grid_with_mean_placement_reorders_the_input():
    """12 vertices in 12 cells of G = 8 over [-1, 1]^3, at binary fractions of the cell size: every coordinate and sum is exact."""
    rng = np.random.default_rng(5)
    cells = rng.permutation(8 ** 3)[:12]
    q = np.stack([cells % 8, (cells // 8) % 8, cells // 64], 1)
    v = (-1.0 + (q + 0.5) * 0.25 + rng.choice([-0.0625, 0.0, 0.03125], (12, 3))).astype(np.float32)
    nrm = np.eye(3, dtype=np.float32)[rng.integers(0, 3, 12)] * rng.choice([-1.0, 1.0], (12, 1)).astype(np.float32)
    col = rng.integers(0, 5, (12, 3)).astype(np.float32) / 4
    f = np.array([rng.permutation(12)[:3] for _ in range(20)], np.int32)
    f = f[np.unique(np.sort(f, 1), axis=0, return_index=True)[1]]     # one face per vertex set: nothing annihilates
    f = np.concatenate([f, np.arange(12, dtype=np.int32).reshape(4, 3)])  # every vertex used
    f = f[np.sort(np.unique(np.sort(f, 1), axis=0, return_index=True)[1])]
    ov, of, on, oc = S.simplify(v, f, nrm, col, 8, S.LO, S.HI, "mean")
    order = np.argsort(cells, kind="stable")
    rank = np.empty(12, np.int64)
    rank[order] = np.arange(12)
    assert np.array_equal(ov.view(np.int32), v[order].view(np.int32))
    assert np.array_equal(on, nrm[order]) and np.array_equal(oc, col[order])
    assert np.array_equal(of, rank[f].astype(np.int32))


def test_invalid_vertices_and_indices_drop_exactly_their_faces():
    v, f, n, _ = (a.copy() for a in S.mesh("sphere"))
    bad_v = [7, 400]
    v[bad_v[0], 1] = np.nan
    v[bad_v[1], 0] = np.inf
    f[10, 2] = len(v)
    f[11, 0] = -1
    f[12, 1] = np.iinfo(np.int32).max
    info = {}
    S.simplify(v, f, n, None, 12, S.LO, S.HI, "quadric", info)
    dropped = np.isin(f, bad_v).any(1)
    dropped[[10, 11, 12]] = True
    assert dropped.sum() > 3
    clean = {}
    v0, f0, n0, _ = S.mesh("sphere")
    S.simplify(v0, f0, n0, None, 12, S.LO, S.HI, "quadric", clean)
    assert np.array_equal(info["keys"] == S.NO_KEY, dropped | (clean["keys"] == S.NO_KEY))
    assert not info["keep"][dropped].any()
    # what remains is the simplification of the mesh without those faces and vertices
    keepf = ~dropped
    a = S.simplify(v, f[keepf], n, None, 12, S.LO, S.HI)
    b = S.simplify(v, f, n, None, 12, S.LO, S.HI)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


def test_runs_of_one_vertex_set():
    v = np.array([[-0.5, -0.5, -0.5], [0.5, -0.5, -0.5], [-0.5, 0.5, 0.5]], np.float32)
    n = np.zeros((3, 3), np.float32)
    a, b = [0, 1, 2], [0, 2, 1]
    f = np.array([a, b, b, a, a, [1, 2, 0], b, a], np.int32)          # 5 against 3: the last two of the majority stay
    info = {}
    ov, of, _, _ = S.simplify(v, f, n, None, 2, S.LO, S.HI, "mean", info)
    assert np.array_equal(np.nonzero(info["keep"])[0], [5, 7])
    assert np.array_equal(of, [[1, 2, 0], [0, 1, 2]]) and len(ov) == 3


def test_argument_checks():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f, n, c = (torch.from_numpy(a.copy()) for a in S.mesh("small"))
    good = E.Mesh(v, f, n, c)
    assert E.check_simplify_args(good, 8, S.LO, S.HI, "quadric") == (8, S.LO, S.HI, S.QUADRIC)
    assert E.check_simplify_args(good._replace(colors=None), 2, S.LO, S.HI, "mean")[3] == S.MEAN
    for grid in (1, 0, -3, E.MAX_RES + 1, 8.0, True, None):
        with pytest.raises(ValueError):
            E.check_simplify_args(good, grid, S.LO, S.HI)
    for placement in ("median", 1, None, "Quadric"):
        with pytest.raises(ValueError):
            E.check_simplify_args(good, 8, S.LO, S.HI, placement)
    for lo, hi in (([0.0] * 3, [0.0] * 3), ([-1, -1, 1], [1, 1, 1]), ([-1, -1], [1, 1]), ([-1, -1, float("nan")], [1, 1, 1])):
        with pytest.raises(ValueError):
            E.check_simplify_args(good, 8, lo, hi)
    bad = [good._replace(verts=v.double()), good._replace(faces=f.long()), good._replace(normals=n[:-1]),
           good._replace(colors=c[:, :2]), good._replace(verts=v.t().contiguous().t()), good._replace(faces=f[:, :2]),
           good._replace(normals=None), good._replace(verts=v.numpy()), (v, f)]
    for m in bad:
        with pytest.raises(ValueError):
            E.check_simplify_args(m, 8, S.LO, S.HI)
    with pytest.raises(ValueError):
        E.check_simplify_grid(-1)
    assert E.check_simplify_grid(0) == 0 and E.check_simplify_grid(E.MAX_RES) == E.MAX_RES


def test_header_section_and_bindings():
    from nerf_meets_mlx_amd import _native
    text = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    start = text.index("mesh simplification (no reference counterpart)")
    section = text[start:text.index("/* ----", start)]
    decl = re.sub(r"/\*.*?\*/", "", "/*" + section, flags=re.S)
    entries = sorted(set(re.findall(r"\b(nerf_simplify_[a-z_]+)\s*\(", decl)))
    assert entries == ["nerf_simplify_cluster", "nerf_simplify_count", "nerf_simplify_workspace_bytes", "nerf_simplify_write"]
    for e in entries:
        assert e in _native.SIGNATURES
    for word in ("Cramer", "det = (a00 c00 + a01 c01) + a02 c02", "Not done"):
        assert word in section
    src = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "Makefile")).read()
    assert "simplify.hip" in src


@pytest.mark.parametrize("G", [2, 512])
@pytest.mark.parametrize("V,F", [(1, 1), (3, 1), (255, 257), (1 << 24, 1 << 24)])
def test_workspace_bytes_region_by_region(V, F, G):
    """nerf_simplify_workspace_bytes in closed form: the regions of the header's workspace in their order, each rounded up to 8
    bytes; nb(n) workgroups of 256 items."""
    from nerf_meets_mlx_amd import _native
    r8 = lambda b: (b + 7) & ~7
    nb = lambda n: (n + 255) // 256
    cells = G ** 3
    W, K = (cells + 63) >> 6, min(V, cells)
    want = (r8(8 * W) + r8(8 * 19 * K) + r8(8 * 4)                               # mask, acc, cnt
            + r8(8 * nb(W)) + r8(8 * nb(K)) + r8(8 * 2 * nb(F)) + r8(8 * nb(F))  # blk_w, blk_c, blk_s, blk_f
            + r8(4 * W) + r8(4 * V) + 3 * r8(4 * K)                              # wpre, vcid, ckey, used, newid
            + r8(4 * (F + 1)) + r8(4 * F) + r8(4 * (F + 1)) + r8(4 * F) + r8(F))  # odd, rid, heads, keep, par
    assert _native.lib().nerf_simplify_workspace_bytes(V, F, G) == want


def test_mesh_tool_stats_know_the_simplifier_kernels(tmp_path, capsys):
    import argparse
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("ngp_mesh_tool", os.path.join(ROOT, "tools", "ngp_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "simplify.hip")).read()
    kernels = sorted(set(re.findall(r"\b(simp_\w+_kernel)\(", src)))
    assert len(kernels) >= 10
    path = tmp_path / "trace.csv"
    with open(path, "w") as fh:
        fh.write('"Kernel_Name","Start_Timestamp","End_Timestamp","Grid_Size_X"\n')
        for i, k in enumerate(kernels):
            for rep in range(2):
                fh.write(f'"void nerf::(anonymous namespace)::{k}(float const*, int)",{1000 * i},{1000 * i + 500 + 1000 * rep},{256 * (i + 1)}\n')
    tool.stats(argparse.Namespace(stats=str(path), from_=None, out=None))
    recs = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert sorted(r["kernel"] for r in recs) == kernels
    assert all(r["launches"] == 2 and r["R"] is None and r["avg_us"] == 1.0 for r in recs)
