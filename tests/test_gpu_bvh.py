"""The mesh BVH on the GPU (csrc/bvh.hip, engine/mesh/distance.py) against the numpy brute force of tests/_distance_ref.py and the
mirror of tests/_bvh_ref.py: squared distances, faces, keys, node boxes and closest points compared as integer bit patterns -- no
tolerance, the rule is exact -- into sentinel-filled outputs that carry one spare row, with a poisoned workspace; then the grid
index on the device and mesh_distance with either index, which must agree field by field."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _bvh_ref as B
from tests import _distance_ref as D
from tests._poison import BIG_BYTES, NAN_BYTES, SENTINEL, bits_equal, poison_, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"


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


def _points(v, f, n=257, seed=5):
    """query_points (one NaN point and points outside the box among them) and the points 100 box widths away."""
    return np.concatenate([D.query_points(v, f, n, seed), B.far_points()])


MESHES = dict(D.MESHES)
MESHES.update({f"small{F}": functools.partial(B.small, F) for F in (0, 1, 3, 4, 5, 8, 9, 17)})
MESHES.update({"all_invalid": B.all_invalid, "doubled": B.doubled})
# for the build alone: 8128 faces, depth 11, so two per-level launches run (the mirror's exact walk would take too long in a query test)
BUILD_MESHES = dict(MESHES, doubled_sphere24=functools.partial(B.doubled, "sphere24"))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(verts, faces, points, dist2, face of the brute force): computed once, shared, read-only."""
    v, f = BUILD_MESHES[name]()
    v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3)
    pts = _points(v, f) if len(v) else np.concatenate([D.query_points(D.cube()[0], D.cube()[1], 257, 5), B.far_points()])
    d2, fc = D.brute_force(pts, v, f)
    for a in (v, f, pts, d2, fc):
        a.setflags(write=False)
    return v, f, pts, d2, fc


class _Tree:
    """nerf_bvh_keys / torch.sort / nerf_bvh_build on numpy inputs with a poisoned workspace and sentinel-filled keys; query() and
    closest() are the other two C calls into sentinel outputs with one spare row."""

    def __init__(self, v, f, pattern=NAN_BYTES, lo=D.LO, hi=D.HI):
        from nerf_meets_mlx_amd import _native as N
        self.N, self.L = N, N.lib()
        self.v0, self.f0 = np.array(v, np.float32).reshape(-1, 3), np.array(f, np.int32).reshape(-1, 3)
        self.tv, self.tf = _dev(self.v0, torch.float32), _dev(self.f0, torch.int32)
        self.V, self.F = len(self.v0), len(self.f0)
        self.box = ((C.c_float * 3)(*lo), (C.c_float * 3)(*hi))
        self.nL, self.P, self.depth, self.launches = B.tree_shape(self.F)
        nbytes = self.L.nerf_bvh_workspace_bytes(self.F)
        assert nbytes == 2 * self.P * 24 + (4 * self.F + 15) // 16 * 16
        self.ws = poison_(torch.empty(nbytes, dtype=torch.uint8, device=DEV), pattern)
        keys = torch.full((self.F + 1,), -77, dtype=torch.int64, device=DEV)
        N.check(self.L.nerf_bvh_keys(N.ptr(self.tv), self.V, N.ptr(self.tf), self.F, *self.box, N.ptr(keys), N.stream()))
        assert int(keys[self.F]) == -77
        self.keys = keys[:self.F].cpu().numpy()
        skeys = torch.sort(keys[:self.F]).values.contiguous()
        N.check(self.L.nerf_bvh_build(N.ptr(self.tv), self.V, N.ptr(self.tf), self.F, N.ptr(skeys), N.ptr(self.ws), N.stream()))
        torch.cuda.synchronize()
        raw = self.ws.cpu().numpy()
        self.nodes = raw[:2 * self.P * 24].view(np.float32).reshape(2 * self.P, 6).copy()
        self.order = raw[2 * self.P * 24:2 * self.P * 24 + 4 * self.F].view(np.int32).copy()
        self.pad = raw[2 * self.P * 24 + 4 * self.F:]
        assert (self.pad == pattern).all()                             # nothing is written behind the order

    def _unchanged(self):
        assert np.array_equal(_bits(self.tv.cpu().numpy()), _bits(self.v0)) and np.array_equal(self.tf.cpu().numpy(), self.f0)

    def query(self, pts):
        N, n = self.N, len(pts)
        tp = _dev(np.asarray(pts, np.float32).reshape(-1, 3), torch.float32)
        d2 = sentinel_(torch.empty(n + 1, dtype=torch.float32, device=DEV))
        fc = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device=DEV)
        before = self.ws.clone()
        N.check(self.L.nerf_bvh_query(N.ptr(tp), n, N.ptr(self.tv), self.V, N.ptr(self.tf), self.F, *self.box, N.ptr(self.ws),
                                      N.ptr(d2), N.ptr(fc), N.stream()))
        torch.cuda.synchronize()
        assert unwritten(d2[n:]) == 1 and int(fc[n]) == SENTINEL and torch.equal(before, self.ws)
        assert np.array_equal(_bits(tp.cpu().numpy()), _bits(np.asarray(pts, np.float32).reshape(-1, 3)))
        self._unchanged()
        return d2[:n].cpu().numpy(), fc[:n].cpu().numpy()

    def closest(self, pts, face):
        N, n = self.N, len(pts)
        tp, tf = _dev(np.asarray(pts, np.float32).reshape(-1, 3), torch.float32), _dev(np.asarray(face, np.int32), torch.int32)
        q = sentinel_(torch.empty(n + 1, 3, dtype=torch.float32, device=DEV))
        N.check(self.L.nerf_closest_points(N.ptr(tp), n, N.ptr(self.tv), self.V, N.ptr(self.tf), self.F, N.ptr(tf), N.ptr(q),
                                           N.stream()))
        torch.cuda.synchronize()
        assert unwritten(q[n:]) == 3 and unwritten(q[:n]) == 0 and np.array_equal(tf.cpu().numpy(), np.asarray(face, np.int32))
        self._unchanged()
        return q[:n].cpu().numpy()


def _assert_same(got, want, what):
    bad = (_bits(got[0]) != _bits(want[0])) | (got[1] != want[1])
    assert not bad.any(), (what, int(bad.sum()), np.nonzero(bad)[0][:6], got[0][bad][:6], want[0][bad][:6], got[1][bad][:6], want[1][bad][:6])


# ------------------------------------------------------------------------------------------------ against the brute force
@pytest.mark.parametrize("name", list(MESHES))
def test_query_matches_the_brute_force_bit_for_bit(name):
    v, f, pts, d2, fc = _case(name)
    assert len(pts) == 264 and np.isnan(pts).any(1).sum() == 1
    fin = np.isfinite(pts).all(1)
    ok = D.corners(v, f)[0]
    for pattern in (NAN_BYTES, BIG_BYTES):
        _assert_same(_Tree(v, f, pattern).query(pts), (d2, fc), (name, pattern))
    assert _bits(d2)[~fin][0] == 0x7FC00000 and fc[~fin][0] == -1
    if not ok.any():                                                  # no valid face: +inf and -1 for every finite point
        assert np.isposinf(d2[fin]).all() and (fc == -1).all()
    else:
        assert np.isfinite(d2[fin]).all() and ok[fc[fin]].all()
    if name == "doubled":                                             # every distance is attained twice: the lower index wins
        assert (fc[fin] < len(f) // 2).all()


@pytest.mark.parametrize("name", ["sphere24", "junk", "spanning", "outside", "small5", "small17", "small0", "all_invalid",
                                  "doubled_sphere24"])
def test_keys_order_and_nodes_match_the_mirror_bit_for_bit(name):
    v, f, _, _, _ = _case(name)
    t = _Tree(v, f, BIG_BYTES)
    if name == "doubled_sphere24":
        assert (t.nL, t.P, t.depth, t.launches) == (2032, 2048, 11, 4)
    assert np.array_equal(t.keys, B.keys(v, f, D.LO, D.HI))
    assert np.array_equal(t.order, B.order(v, f, D.LO, D.HI))
    assert np.array_equal(_bits(t.nodes), _bits(B.nodes(v, f, D.LO, D.HI)))
    assert t.launches <= 23 and t.depth <= 22


def test_face_order_chunks_and_repeats():
    v, f, pts, d2, fc = _case("sphere24")
    t = _Tree(v, f)
    first = t.query(pts)
    again = t.query(pts)
    assert np.array_equal(_bits(first[0]), _bits(again[0])) and np.array_equal(first[1], again[1])
    a, b = t.query(pts[:100]), t.query(pts[100:])                      # two ragged chunks against one tree
    assert np.array_equal(_bits(np.concatenate([a[0], b[0]])), _bits(first[0]))
    assert np.array_equal(np.concatenate([a[1], b[1]]), first[1])
    perm = np.random.default_rng(9).permutation(len(f))
    pd, pf = _Tree(v, f[perm], BIG_BYTES).query(pts)
    assert np.array_equal(_bits(pd), _bits(d2))                        # the same distance bits under a permuted face list
    fin = pf >= 0
    # the face maps through the permutation, up to ties: the face answered attains the distance, and where the brute force's
    # face is the only one that does, it is that face
    assert np.array_equal(_bits(D.point_triangle_d2(pts[fin], *(v[f[perm][pf[fin]][:, k]] for k in range(3)))), _bits(pd[fin]))
    pd2, pf2 = D.brute_force(pts, v, f[perm])
    assert np.array_equal(pf, pf2) and np.array_equal(_bits(pd), _bits(pd2))


def test_engine_bvh_sorted_one_shot_and_the_grid_on_the_device():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f, pts, d2, fc = _case("sphere24")
    m, tp = _mesh(v, f), _dev(pts, torch.float32)
    bvh = E.MeshBVH(m, D.LO, D.HI)
    assert (bvh.leaves, bvh.P) == B.tree_shape(len(f))[:2]
    assert np.array_equal(bvh.order.cpu().numpy(), B.order(v, f, D.LO, D.HI))
    assert np.array_equal(_bits(bvh.nodes.cpu().numpy()), _bits(B.nodes(v, f, D.LO, D.HI)))
    gd, gf = E.MeshIndex(m, D.LO, D.HI).query(tp)                      # the default grid, on the device
    for sort in (False, True, None):
        bd, bf = bvh.query(tp, sort=sort)
        _assert_same((bd.cpu().numpy(), bf.cpu().numpy()), (d2, fc), ("engine", sort))
        assert bits_equal(bd, gd) and torch.equal(bf, gf)
    od, of = E.point_mesh_distance(tp, m, D.LO, D.HI, index="bvh")
    _assert_same((od.cpu().numpy(), of.cpu().numpy()), (d2, fc), "one shot")
    e = bvh.query(tp[:0])
    assert e[0].shape == (0,) and e[1].shape == (0,) and e[1].dtype == torch.int32
    with pytest.raises(ValueError):
        bvh.query(tp.double())
    with pytest.raises(ValueError):
        bvh.query(tp.cpu())
    with pytest.raises(ValueError):
        E.point_mesh_distance(tp, m, D.LO, D.HI, index="octree")
    empty = E.MeshBVH(_mesh(v, np.zeros((0, 3), np.int32)), D.LO, D.HI)
    ed, ef = empty.query(tp)
    fin = np.isfinite(pts).all(1)
    assert empty.P == 1 and np.isposinf(ed.cpu().numpy()[fin]).all() and (ef.cpu().numpy() == -1).all()


# ------------------------------------------------------------------------------------------------ the closest point
@pytest.mark.parametrize("name", ["sphere24", "junk", "outside", "doubled"])
def test_closest_points_match_the_mirror_and_recompute_dist2(name):
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f, pts, d2, fc = _case(name)
    t = _Tree(v, f)
    ok = D.corners(v, f)[0]
    odd = np.array([-1, len(f), -7, 1 << 30] + list(np.nonzero(~ok)[0][:3]), np.int32)
    face = np.concatenate([fc, odd]).astype(np.int32)
    p = np.concatenate([pts, pts[:len(odd)]])
    q = t.closest(p, face)
    assert np.array_equal(_bits(q), _bits(B.closest(p, v, f, face)))
    hit = fc >= 0
    assert np.array_equal(_bits(B.dist2_of(pts, q[:len(pts)])[hit]), _bits(d2[hit]))       # dot(p - q, p - q) is dist2, bit for bit
    assert (_bits(q[len(pts):]) == 0x7FC00000).all() and (_bits(q[:len(pts)][~hit]) == 0x7FC00000).all()
    m, tp = _mesh(v, f), _dev(pts, torch.float32)
    bd, bf = E.MeshBVH(m, D.LO, D.HI).query(tp)
    eq = E.closest_points(m, tp, bf)
    assert eq.shape == (len(pts), 3) and np.array_equal(_bits(eq.cpu().numpy()), _bits(q[:len(pts)]))
    d = tp - eq
    again = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    keep = torch.from_numpy(hit).to(DEV)
    assert bits_equal(again[keep], bd[keep])


# ------------------------------------------------------------------------------------------------ in geometric terms
DELTA = 2.0 ** -4


def test_mesh_distance_with_either_index_on_a_cube_and_its_shifted_copy():
    from nerf_meets_mlx_amd.engine import mesh as E
    (va, fa), (vb, fb) = D.cube(), D.cube(DELTA)
    a, b = _mesh(va, fa), _mesh(vb, fb)
    n = 4096
    r = E.mesh_distance(a, b, n, D.LO, D.HI, seed=3, tau=2 * DELTA, index="bvh")
    g = E.mesh_distance(a, b, n, D.LO, D.HI, seed=3, tau=2 * DELTA, index="grid")
    d = E.mesh_distance(a, b, n, D.LO, D.HI, seed=3, tau=2 * DELTA)
    # the known distances (tests/test_gpu_distance.py derives them): every point of one cube is within delta of the other
    assert r.symmetric.max <= DELTA and r.a_to_b.max <= DELTA and r.b_to_a.max <= DELTA
    assert 0 < r.symmetric.mean <= r.symmetric.rms <= r.symmetric.max
    assert (r.precision, r.recall, r.fscore) == (1.0, 1.0, 1.0)
    assert bool((r.dist2_ab.double().sqrt() <= DELTA).all()) and bool((r.dist2_ba.double().sqrt() <= DELTA).all())
    for other in (g, d):
        assert (r.a_to_b, r.b_to_a, r.symmetric, r.precision, r.recall, r.fscore) == \
            (other.a_to_b, other.b_to_a, other.symmetric, other.precision, other.recall, other.fscore)
        for x, y in ((r.points_a, other.points_a), (r.points_b, other.points_b), (r.dist2_ab, other.dist2_ab), (r.dist2_ba, other.dist2_ba)):
            assert bits_equal(x, y)
        assert torch.equal(r.face_ab, other.face_ab) and torch.equal(r.face_ba, other.face_ba)
    with pytest.raises(ValueError, match="index"):
        E.mesh_distance(a, b, n, D.LO, D.HI, index="kd")
