"""Mesh distance on the GPU (csrc/distance.hip, engine/mesh/distance.py, Trainer.mesh_distance) against the numpy mirror of
tests/_distance_ref.py: squared distances, faces and sampled points compared as integer bit patterns -- no tolerance, the rule is
exact -- into sentinel-filled outputs that carry one spare row, with a poisoned workspace, at every grid size; then the metric in
geometric terms on a cube and its shifted copy, where the answers are known without any reference."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _distance_ref as D
from tests import _smooth_ref as S
from tests._poison import BIG_BYTES, NAN_BYTES, SENTINEL, bits_equal, poison_, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRIDS = (1, 2, 3, 16, 33)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, order="C")).to(device=DEV, dtype=dtype).contiguous()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _mesh(v, f):
    from nerf_meets_mlx_amd.engine import mesh as E
    tv = _dev(v, torch.float32).reshape(-1, 3)
    return E.Mesh(tv, _dev(f, torch.int32).reshape(-1, 3), torch.zeros_like(tv))


@functools.lru_cache(maxsize=None)
def _case(name, n, seed=5):
    """(verts, faces, points, dist2, face of the brute force): computed once, shared, read-only."""
    v, f = D.MESHES[name]()
    pts = D.query_points(v, f, n, seed)
    d2, fc = D.brute_force(pts, v, f)
    for a in (pts, d2, fc):
        a.setflags(write=False)
    return v, f, pts, d2, fc


class _Index:
    """nerf_meshdist_count / _build on numpy inputs with a poisoned workspace and sentinel-filled entries; query() is the third C
    call into sentinel outputs with one spare row."""

    def __init__(self, v, f, G, pattern=NAN_BYTES, lo=D.LO, hi=D.HI):
        from nerf_meets_mlx_amd import _native as N
        self.N, self.L, self.G = N, N.lib(), G
        self.v0, self.f0 = np.array(v, np.float32).reshape(-1, 3), np.array(f, np.int32).reshape(-1, 3)
        self.tv, self.tf = _dev(self.v0, torch.float32), _dev(self.f0, torch.int32)
        self.V, self.F = len(self.v0), len(self.f0)
        self.box = ((C.c_float * 3)(*lo), (C.c_float * 3)(*hi))
        nbytes = self.L.nerf_meshdist_workspace_bytes(self.F, G)
        assert nbytes > 0
        self.ws = poison_(torch.empty(nbytes, dtype=torch.uint8, device=DEV), pattern)
        tot = torch.full((2,), -77, dtype=torch.int64, device=DEV)
        N.check(self.L.nerf_meshdist_count(N.ptr(self.tv), self.V, N.ptr(self.tf), self.F, *self.box, G, N.ptr(self.ws), N.ptr(tot),
                                           N.stream()))
        self.E = int(tot[0])
        assert int(tot[1]) == -77 and self.E >= 0
        self.ent = torch.full((self.E + 1,), -5, dtype=torch.int32, device=DEV)
        N.check(self.L.nerf_meshdist_build(N.ptr(self.tv), self.V, N.ptr(self.tf), self.F, *self.box, G, N.ptr(self.ws),
                                           N.ptr(self.ent), self.E, N.stream()))
        ent = self.ent.cpu().numpy()
        assert ent[self.E] == -5 and (ent[:self.E] >= 0).all() and (ent[:self.E] < max(self.F, 1)).all()
        self.entries = ent[:self.E]

    def query(self, pts):
        N, n = self.N, len(pts)
        tp = _dev(np.asarray(pts, np.float32).reshape(-1, 3), torch.float32)
        d2 = sentinel_(torch.empty(n + 1, dtype=torch.float32, device=DEV))
        fc = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device=DEV)
        N.check(self.L.nerf_meshdist_query(N.ptr(tp), n, N.ptr(self.tv), self.V, N.ptr(self.tf), self.F, *self.box, self.G,
                                           N.ptr(self.ws), N.ptr(self.ent), self.E, N.ptr(d2), N.ptr(fc), N.stream()))
        torch.cuda.synchronize()
        assert unwritten(d2[n:]) == 1 and int(fc[n]) == SENTINEL
        assert np.array_equal(_bits(tp.cpu().numpy()), _bits(np.asarray(pts, np.float32).reshape(-1, 3)))
        assert np.array_equal(_bits(self.tv.cpu().numpy()), _bits(self.v0)) and np.array_equal(self.tf.cpu().numpy(), self.f0)
        return d2[:n].cpu().numpy(), fc[:n].cpu().numpy()


def _assert_same(got, want, what):
    bad = (_bits(got[0]) != _bits(want[0])) | (got[1] != want[1])
    assert not bad.any(), (what, int(bad.sum()), np.nonzero(bad)[0][:6], got[0][bad][:6], want[0][bad][:6], got[1][bad][:6], want[1][bad][:6])


# ------------------------------------------------------------------------------------------------ against the brute force
CASES = [(name, 257) for name in D.MESHES] + [("sphere12", n) for n in (1, 63, 64, 65, 3001)]


@pytest.mark.parametrize("name,n", CASES)
def test_query_matches_the_brute_force_bit_for_bit_at_every_grid(name, n):
    v, f, pts, d2, fc = _case(name, n)
    assert len(pts) == n
    if n >= 257:                                                      # the point set holds what it should
        assert np.isnan(pts).any(1).sum() == 1 and (d2[np.isfinite(pts).all(1)] == 0).sum() >= min(len(v), 100) // 2
        assert ((pts < np.array(D.LO)) | (pts > np.array(D.HI))).any(1).sum() >= 7
    for k, G in enumerate(GRIDS + (D.default_grid(len(f)),)):
        idx = _Index(v, f, G, (NAN_BYTES, BIG_BYTES)[k % 2])
        _assert_same(idx.query(pts), (d2, fc), (name, n, G))
        if name == "spanning" and G > 1:                              # more entries than faces, and no cell is empty
            assert idx.E > len(f) and np.bincount(idx.entries, minlength=len(f))[0] == G ** 3
        if G == 1:
            assert idx.E == int(D.corners(v, f)[0].sum())             # the brute-force scan: every valid face once


@pytest.mark.parametrize("G", [6, 7])
def test_query_at_cell_counts_around_one_workgroup(G):
    """The cell offsets come from csrc/scan.h's counts-to-offsets pair, 256 cells a workgroup: 216 cells sit just under one
    workgroup and 343 just over (one cell is GRIDS[0]; no cube is 256).  The query against the brute force, and the offsets
    themselves: an exclusive scan that ends at E, every cursor left at the end of its cell by the fill."""
    v, f, pts, d2, fc = _case("sphere12", 257)
    idx = _Index(v, f, G)
    _assert_same(idx.query(pts), (d2, fc), ("sphere12", 257, G))
    cells, nblk = G ** 3, -(-G ** 3 // 256)
    at = 8 * nblk + 16                                                # behind blk [nblk], total and scale
    off = idx.ws[at:at + 4 * (cells + 1)].view(torch.int32).cpu().numpy()
    cur = idx.ws[at + 8 * ((cells + 2) // 2):][:4 * cells].view(torch.int32).cpu().numpy()      # off's cells + 1 ints, rounded to 8 B
    assert off[0] == 0 and off[cells] == idx.E and (np.diff(off) >= 0).all() and np.array_equal(cur, off[1:])


def test_the_nan_point_an_empty_mesh_and_a_mesh_of_invalid_faces():
    v, f, pts, d2, fc = _case("junk", 257)
    i = int(np.nonzero(np.isnan(pts).any(1))[0][0])
    got = _Index(v, f, 16).query(pts)
    assert _bits(got[0])[i] == 0x7FC00000 and got[1][i] == -1
    ok = D.corners(v, f)[0]
    for vv, ff in ((v, f[~ok]), (v, np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))):
        for G in (1, 3):
            idx = _Index(vv, ff, G)
            gd, gf = idx.query(pts)
            fin = np.isfinite(pts).all(1)
            assert idx.E == 0 and np.isposinf(gd[fin]).all() and (gf == -1).all() and np.isnan(gd[~fin]).all()


def test_face_order_chunks_and_repeats():
    v, f, pts, d2, fc = _case("sphere24", 257)
    idx = _Index(v, f, 16)
    first = idx.query(pts)
    again = idx.query(pts)
    assert np.array_equal(_bits(first[0]), _bits(again[0])) and np.array_equal(first[1], again[1])
    a, b = idx.query(pts[:100]), idx.query(pts[100:])                  # two ragged chunks against one index
    assert np.array_equal(_bits(np.concatenate([a[0], b[0]])), _bits(first[0]))
    assert np.array_equal(np.concatenate([a[1], b[1]]), first[1])
    perm = np.random.default_rng(9).permutation(len(f))
    pd, pf = _Index(v, f[perm], 16, BIG_BYTES).query(pts)
    assert np.array_equal(_bits(pd), _bits(d2))                        # the same distance bits under a permuted face list
    fin = pf >= 0
    assert np.array_equal(_bits(D.point_triangle_d2(pts[fin], *(v[f[perm][pf[fin]][:, k]] for k in range(3)))), _bits(pd[fin]))


def test_engine_index_query_sorted_and_one_shot():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f, pts, d2, fc = _case("sphere24", 257)
    m, tp = _mesh(v, f), _dev(pts, torch.float32)
    idx = E.MeshIndex(m, D.LO, D.HI)
    assert idx.grid == D.default_grid(len(f)) == 11 and idx.entries >= len(f)
    for sort in (False, True, None):
        gd, gf = idx.query(tp, sort=sort)
        _assert_same((gd.cpu().numpy(), gf.cpu().numpy()), (d2, fc), ("engine", sort))
    gd, gf = E.point_mesh_distance(tp, m, D.LO, D.HI, grid=1)
    _assert_same((gd.cpu().numpy(), gf.cpu().numpy()), (d2, fc), "one shot, grid 1")
    e = idx.query(tp[:0])
    assert e[0].shape == (0,) and e[1].shape == (0,) and e[1].dtype == torch.int32
    with pytest.raises(ValueError):
        idx.query(tp.double())
    with pytest.raises(ValueError):
        idx.query(tp.cpu())
    with pytest.raises(ValueError):
        E.MeshIndex(m, D.LO, D.HI, grid=0)


# ------------------------------------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("name", ["sphere12", "junk", "outside"])
def test_sampler_matches_the_mirror_bit_for_bit(name):
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    v, f = D.MESHES[name]()
    ok = D.corners(v, f)[0]
    tv, tf = _dev(v, torch.float32), _dev(f, torch.int32)
    V, F = len(v), len(f)
    lo, hi = (C.c_float * 3)(*D.LO), (C.c_float * 3)(*D.HI)
    want_cdf = D.cdf(v, f, D.LO, D.HI)
    for pattern in (NAN_BYTES, BIG_BYTES):
        ws = poison_(torch.empty(L.nerf_surface_cdf_workspace_bytes(F), dtype=torch.uint8, device=DEV), pattern)
        cdf = torch.full((F + 1,), -9, dtype=torch.int64, device=DEV)
        N.check(L.nerf_surface_cdf(N.ptr(tv), V, N.ptr(tf), F, lo, hi, N.ptr(ws), N.ptr(cdf), N.stream()))
        assert np.array_equal(cdf[:F].cpu().numpy(), want_cdf) and int(cdf[F]) == -9
    total = int(want_cdf[-1])
    for n in (1, 64, 65, 1000):
        for seed in (0, 7):
            wp, wf, _ = D.sample(v, f, n, D.LO, D.HI, seed)
            pts = sentinel_(torch.empty(n + 1, 3, dtype=torch.float32, device=DEV))
            fc = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device=DEV)
            N.check(L.nerf_surface_sample(N.ptr(tv), V, N.ptr(tf), F, N.ptr(cdf), total, n, seed, N.ptr(pts), N.ptr(fc), N.stream()))
            torch.cuda.synchronize()
            assert unwritten(pts[n:]) == 3 and int(fc[n]) == SENTINEL
            gp, gf = pts[:n].cpu().numpy(), fc[:n].cpu().numpy()
            assert np.array_equal(gf, wf) and np.array_equal(_bits(gp), _bits(wp)), (name, n, seed)
            assert ok[gf].all()                                       # every drawn face is valid
    assert np.array_equal(_bits(tv.cpu().numpy()), _bits(v)) and np.array_equal(tf.cpu().numpy(), f)


def test_engine_sampler_empty_and_refused():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = S.sphere(12)
    m = _mesh(v, f)
    wp, wf, _ = D.sample(v, f, 65, D.LO, D.HI, 7)
    gp, gf = E.sample_surface(m, 65, D.LO, D.HI, seed=7)
    assert gf.dtype == torch.int32 and np.array_equal(gf.cpu().numpy(), wf) and np.array_equal(_bits(gp.cpu().numpy()), _bits(wp))
    p0, f0 = E.sample_surface(m, 0, D.LO, D.HI)
    assert p0.shape == (0, 3) and f0.shape == (0,) and p0.dtype == torch.float32
    flat = _mesh(np.array([[0, 0, 1], [1, 0, 1], [2, 0, 1]], np.float32), np.array([[0, 1, 2], [0, 0, 1], [0, 1, 5]], np.int32))
    for bad in (flat, _mesh(v, np.zeros((0, 3), np.int32))):
        with pytest.raises(ValueError, match="no area"):
            E.sample_surface(bad, 4, D.LO, D.HI)
        assert E.sample_surface(bad, 0, D.LO, D.HI)[0].shape == (0, 3)


# ------------------------------------------------------------------------------------------------ in geometric terms
DELTA = 2.0 ** -4
# A sampled point is (a + u1 e1) + u2 e2 in float32: four roundings, each at most 2^-24 of a value of magnitude at most 2 (the
# cubes' coordinates lie in [-0.5, 2]), so every coordinate is within 4 * 2^-24 * 2 = 2^-21 of the face.  The float32 distance is
# that of a point within 64 * 2^-24 * S of the triangle (include/nerf_hip.h "mesh distance", query), S = 2 here: 2^-17.
ROUND = 2.0 ** -17 + 2.0 ** -21


def test_a_cube_and_its_shifted_copy():
    from nerf_meets_mlx_amd.engine import mesh as E
    (va, fa), (vb, fb) = D.cube(), D.cube(DELTA)
    a, b = _mesh(va, fa), _mesh(vb, fb)
    n = 4096
    r = E.mesh_distance(a, b, n, D.LO, D.HI, seed=3, tau=2 * DELTA)
    for pts, face, d2 in ((r.points_a, E.sample_surface(a, n, D.LO, D.HI, 3)[1], r.dist2_ab),
                          (r.points_b, E.sample_surface(b, n, D.LO, D.HI, 3)[1], r.dist2_ba)):
        d = d2.double().sqrt().cpu().numpy()
        print("cube: max distance", d.max(), "delta", DELTA)
        # Every point of one cube is within delta of the other, with no allowance: the cubes differ along x only, where every
        # coordinate is a binary fraction and the faces' edge vectors have a zero x component or an exact one, so the x offset
        # of a sample from the other cube's planes is exact; what the other axes add is below half an ulp of delta^2.
        assert (d <= DELTA).all()
        on_x = np.isin(face.cpu().numpy(), [8, 9, 10, 11])              # the faces x = -0.5 and x = +0.5 (+ delta)
        assert 0.2 * n < on_x.sum() < 0.47 * n                          # a third of the area
        far = np.abs(d[on_x] - DELTA) <= ROUND                          # at delta, unless an edge of the other cube is nearer
        y, z = pts[:, 1].cpu().numpy()[on_x], pts[:, 2].cpu().numpy()[on_x]
        inner = (np.abs(y - 0.75) < 0.5 - DELTA) & (np.abs(z - 1.5) < 0.5 - DELTA)
        # one of the two x-faces looks at the other cube's parallel face at exactly delta, the other lies inside the other cube,
        # delta from that same kind of face
        assert far[inner].all() and inner.sum() > 0.1 * n
    assert r.symmetric.max <= DELTA and r.a_to_b.max <= DELTA and r.b_to_a.max <= DELTA          # the Hausdorff distance
    assert 0 < r.symmetric.mean <= r.symmetric.rms <= r.symmetric.max
    assert (r.precision, r.recall, r.fscore) == (1.0, 1.0, 1.0)
    tight = E.mesh_distance(a, b, n, D.LO, D.HI, seed=3, tau=DELTA / 4)
    assert 0 < tight.precision < 1 and 0 < tight.recall < 1 and 0 < tight.fscore < 1
    assert bits_equal(tight.dist2_ab, r.dist2_ab) and torch.equal(tight.face_ab, r.face_ab)
    same = E.mesh_distance(a, a, n, D.LO, D.HI, seed=3)
    assert same.symmetric.max <= ROUND and same.precision is None and same.fscore is None
    assert bool((same.dist2_ab.double().sqrt() <= ROUND).all()) and bool((same.dist2_ba.double().sqrt() <= ROUND).all())


def test_trainer_mesh_distance():
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine import mesh as E
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    imgs, poses, _, _, K = synthetic.make_dataset(8, 8, 2, seed=0, device=DEV)
    tr = Trainer(imgs, poses, K, N_rand=64, n_depth_samples=16, N_importance=16, seed=4, device=DEV)
    box = ([-1.0] * 3, [1.0] * 3)
    vol = tr.density_volume(16, box)
    thr = float(vol.reshape(-1).quantile(0.7))
    raw = tr.extract_mesh(resolution=16, threshold=thr, aabb=box, colors=False)
    simp = tr.extract_mesh(resolution=16, threshold=thr, aabb=box, colors=False, simplify_grid=8)
    assert 0 < simp.faces.shape[0] < raw.faces.shape[0]
    got = tr.mesh_distance(simp, raw, n=2048, tau=0.25, seed=1, aabb=box)
    want = E.mesh_distance(simp, raw, 2048, *box, seed=1, tau=0.25)
    print("simplified (G = 8) against the R = 16 mesh:", got.a_to_b, got.b_to_a, got.fscore)
    for s in (got.a_to_b, got.b_to_a, got.symmetric):
        assert all(np.isfinite(x) and x >= 0 for x in s)
    assert 0.0 <= got.fscore <= 1.0 and got.symmetric.max > 0
    assert bits_equal(got.dist2_ab, want.dist2_ab) and bits_equal(got.dist2_ba, want.dist2_ba)
    assert torch.equal(got.face_ab, want.face_ab) and torch.equal(got.face_ba, want.face_ba)
    with pytest.raises(ValueError):
        tr.mesh_distance(simp, raw, n=2048)                             # this trainer's field has no box of its own
    with pytest.raises(ValueError):
        tr.mesh_distance(simp, raw, n=2048, tau=-1.0, aabb=box)
