"""The mesh winding number on the GPU (csrc/winding.hip, engine/mesh/winding.py) against the numpy mirror of tests/_winding_ref.py:
the moments and the visit counters compared bit for bit, the winding numbers within the one difference there is -- the device's
float64 atan2, once per face evaluated exactly -- into sentinel-filled outputs that carry one spare row, with poisoned workspaces;
then chunks, repeats, the sorted query and a permuted face list, the volume and the remesh of an open cube, and the signed
distance.

The cap: |w - w_mirror| <= faces evaluated * 2^-48.  One term is 2 atan2 / (4 pi), so 2^-48 of a turn allows atan2 an error of
2 pi 2^-48 = 2^-45.3, some fifty units in the last place of pi (2^-51 each); the sums on either side add what they are given in the
same order with the same roundings apart from that.  It is nine orders of magnitude below the dipole's error.  Where no face was
evaluated the two must be equal."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _bvh_ref as B
from tests import _distance_ref as D
from tests import _mesh_ref as M
from tests import _winding_ref as W
from tests._poison import BIG_BYTES, NAN_BYTES, SENTINEL, bits_equal, poison_

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 2.0 ** -48
BETAS = (np.inf, 2.0, 1.0)
W_SENTINEL = 0x7FF5A5A5A5A5A5A5                                       # a float64 NaN no kernel writes
SPARE = 32                                                            # poisoned bytes behind the moments: never written


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, order="C")).to(device=DEV, dtype=dtype).contiguous()


def _mesh(v, f):
    from nerf_meets_mlx_amd.engine import mesh as E
    tv = _dev(np.asarray(v, np.float32).reshape(-1, 3), torch.float32)
    return E.Mesh(tv, _dev(np.asarray(f, np.int32).reshape(-1, 3), torch.int32), torch.zeros_like(tv))


MESHES = dict(D.MESHES)
MESHES.update({f"small{F}": functools.partial(B.small, F) for F in (0, 1, 3, 4, 5, 8, 9, 17)})
MESHES.update({"all_invalid": B.all_invalid, "doubled": B.doubled})
# for the build alone: 8128 faces, depth 11, so two per-level launches run (the mirror's exact walk would take too long in a query test)
BUILD_MESHES = dict(MESHES, doubled_sphere24=functools.partial(B.doubled, "sphere24"))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(verts, faces, points, the mirror): computed once, shared, read-only.  The points: query_points (one NaN point and points
    outside the box among them) and the points 100 box widths away."""
    v, f = BUILD_MESHES[name]()
    v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3)
    src = (v, f) if len(v) else D.cube()
    pts = np.concatenate([D.query_points(src[0], src[1], 257, 5), B.far_points()])
    wd = W.Winding(v, f)
    for a in (v, f, pts, wd.moments):
        a.setflags(write=False)
    return v, f, pts, wd


@functools.lru_cache(maxsize=None)
def _mirror(name, beta):
    """(the points' indices, w, visits) of the mirror's walk; at beta = inf on sphere24 a subset of 32 points, the NaN one among
    them, for every point visits every face."""
    _, _, pts, wd = _case(name)
    idx = np.arange(len(pts))
    if name == "sphere24" and np.isinf(beta):
        idx = np.concatenate([idx[::9][:31], np.nonzero(~np.isfinite(pts).all(1))[0][:1]])
    w, visits = wd.query(pts[idx], beta)
    return idx, w, visits


class _Wind:
    """MeshBVH of the engine, then nerf_winding_build on a poisoned workspace; query() is nerf_winding_query into sentinel outputs
    with one spare row, and checks that it changed neither workspace nor any input."""

    def __init__(self, v, f, pattern=NAN_BYTES):
        from nerf_meets_mlx_amd import _native as N
        from nerf_meets_mlx_amd.engine import mesh as E
        self.N, self.L = N, N.lib()
        self.v0, self.f0 = np.array(v, np.float32).reshape(-1, 3), np.array(f, np.int32).reshape(-1, 3)
        self.mesh = _mesh(self.v0, self.f0)
        self.V, self.F = len(self.v0), len(self.f0)
        self.bvh = E.MeshBVH(self.mesh, D.LO, D.HI)
        self.P = self.bvh.P
        nbytes = self.L.nerf_winding_workspace_bytes(self.F)
        assert nbytes == 2 * self.P * 96
        self.pattern = pattern
        self.ws = poison_(torch.empty(nbytes + SPARE, dtype=torch.uint8, device=DEV), pattern)
        N.check(self.L.nerf_winding_build(N.ptr(self.mesh.verts), self.V, N.ptr(self.mesh.faces), self.F, N.ptr(self.bvh._ws),
                                          N.ptr(self.ws), N.stream()))
        torch.cuda.synchronize()
        raw = self.ws.cpu().numpy()
        assert (raw[nbytes:] == pattern).all()                         # nothing is written behind the moments
        self.raw = raw[:nbytes]
        self.moments = raw[:nbytes].view(np.float64).reshape(2 * self.P, 12).copy()

    def query(self, pts, beta):
        N, n = self.N, len(pts)
        p0 = np.asarray(pts, np.float32).reshape(-1, 3)
        tp = _dev(p0, torch.float32)
        w = torch.full((n + 1,), W_SENTINEL, dtype=torch.int64, device=DEV).view(torch.float64)
        visits = torch.full((n + 1, 2), SENTINEL, dtype=torch.int32, device=DEV)
        before, bvh_before = self.ws.clone(), self.bvh._ws.clone()
        N.check(self.L.nerf_winding_query(N.ptr(tp), n, N.ptr(self.mesh.verts), self.V, N.ptr(self.mesh.faces), self.F,
                                          N.ptr(self.bvh._ws), N.ptr(self.ws), float(beta), N.ptr(w), N.ptr(visits), N.stream()))
        torch.cuda.synchronize()
        assert int(w.view(torch.int64)[n]) == W_SENTINEL and (visits[n] == SENTINEL).all()                  # the spare row
        assert not bool((w.view(torch.int64)[:n] == W_SENTINEL).any()) and not bool((visits[:n] == SENTINEL).any())
        assert torch.equal(before, self.ws) and torch.equal(bvh_before, self.bvh._ws)
        assert np.array_equal(tp.cpu().numpy().view(np.int32), p0.view(np.int32))
        assert np.array_equal(self.mesh.verts.cpu().numpy().view(np.int32), self.v0.view(np.int32))
        assert np.array_equal(self.mesh.faces.cpu().numpy(), self.f0)
        return w[:n].cpu().numpy(), visits[:n].cpu().numpy()


def _assert_close(got, want, what):
    """visits bit for bit; w within faces * 2^-48, equal where no face was evaluated, the same NaN bits.  Returns the largest
    difference."""
    (gw, gv), (ww, wv) = got, want
    assert gv.dtype == np.int32 and np.array_equal(gv, wv), (what, np.nonzero((gv != wv).any(1))[0][:6])
    nan = np.isnan(ww)
    assert np.array_equal(np.isnan(gw), nan) and (gw[nan].view(np.int64) == 0x7FF8000000000000).all() and not gv[nan].any(), what
    diff = np.abs(gw[~nan] - ww[~nan])
    bad = diff > wv[~nan, 0] * CAP
    assert not bad.any(), (what, int(bad.sum()), diff.max(), np.nonzero(bad)[0][:6])
    return float(diff.max()) if len(diff) else 0.0


# ------------------------------------------------------------------------------------------------ against the mirror
@pytest.mark.parametrize("name", list(BUILD_MESHES))
def test_moments_match_the_mirror_bit_for_bit(name):
    v, f, _, wd = _case(name)
    for pattern in (NAN_BYTES, BIG_BYTES):
        t = _Wind(v, f, pattern)
        if len(f) == 0:                                                # nothing is launched: the workspace is not touched
            assert (t.raw == pattern).all()
            continue
        assert t.moments.shape == wd.moments.shape
        bad = t.moments.view(np.int64) != wd.moments.view(np.int64)
        assert not bad.any(), (name, pattern, np.argwhere(bad)[:6], t.moments[bad][:6], wd.moments[bad][:6])
    if name == "sphere24":
        assert wd.tree.depth == 10 and wd.tree.launches == 3          # the per-level launch runs
    if name == "doubled_sphere24":
        assert wd.tree.depth == 11 and wd.tree.launches == 4          # twice


@pytest.mark.parametrize("name", list(MESHES))
def test_query_matches_the_mirror(name):
    v, f, pts, wd = _case(name)
    assert len(pts) == 264 and np.isnan(pts).any(1).sum() == 1
    worst = 0.0
    for pattern in (NAN_BYTES, BIG_BYTES):
        t = _Wind(v, f, pattern)
        for beta in BETAS:
            idx, ww, wv = _mirror(name, beta)
            worst = max(worst, _assert_close(t.query(pts[idx], beta), (ww, wv), (name, pattern, beta)))
    print(name, "largest |w - w_mirror|", worst)
    fin = np.isfinite(pts).all(1)
    _, ww, wv = _mirror(name, 2.0)
    if wd.valid == 0:                                                 # no valid face: (0, 0, 0) for every finite point
        assert (ww[fin] == 0.0).all() and not wv.any()
    else:
        idx, _, vinf = _mirror(name, np.inf)
        assert (vinf[np.isfinite(pts[idx]).all(1)] == (wd.valid, 0)).all()


# ------------------------------------------------------------------------------------------------ robustness
def test_chunks_repeats_and_the_sorted_query():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f, pts, _ = _case("sphere24")
    t = _Wind(v, f)
    first = t.query(pts, 2.0)
    again = t.query(pts, 2.0)
    assert np.array_equal(first[0].view(np.int64), again[0].view(np.int64)) and np.array_equal(first[1], again[1])
    a, b, c = t.query(pts[:100], 2.0), t.query(pts[100:101], 2.0), t.query(pts[101:], 2.0)      # ragged chunks against one build
    assert np.array_equal(np.concatenate([a[0], b[0], c[0]]).view(np.int64), first[0].view(np.int64))
    assert np.array_equal(np.concatenate([a[1], b[1], c[1]]), first[1])
    m, tp = t.mesh, _dev(pts, torch.float32)
    wd = E.MeshWinding(m, D.LO, D.HI)
    assert np.array_equal(wd.moments.cpu().numpy().view(np.int64), t.moments.view(np.int64))
    assert wd.moments.shape == (2 * wd.P, E.WINDING_NODE_DOUBLES) and wd.bvh.P == wd.P
    ref = None
    for sort in (False, True, None):
        for beta in (2.0, float("inf")):
            w, visits = wd.query(tp, beta, sort=sort)
            assert w.dtype == torch.float64 and visits.dtype == torch.int32 and visits.shape == (len(pts), 2)
            if beta == 2.0:
                assert np.array_equal(w.cpu().numpy().view(np.int64), first[0].view(np.int64))
                assert np.array_equal(visits.cpu().numpy(), first[1])
            else:
                ref = ref or (w, visits)
                assert torch.equal(w.view(torch.int64), ref[0].view(torch.int64)) and torch.equal(visits, ref[1])
    shared = E.MeshWinding(m, D.LO, D.HI, bvh=wd.bvh)                  # a hierarchy the caller has already
    w, visits = shared.query(tp, 2.0)
    assert torch.equal(w.view(torch.int64), wd.query(tp, 2.0)[0].view(torch.int64)) and shared.bvh is wd.bvh
    one, _ = E.winding_number(tp, m, D.LO, D.HI)
    assert torch.equal(one.view(torch.int64), w.view(torch.int64))
    e = wd.query(tp[:0])
    assert e[0].shape == (0,) and e[1].shape == (0, 2)
    with pytest.raises(ValueError):
        wd.query(tp.double())
    with pytest.raises(ValueError):
        wd.query(tp.cpu())
    with pytest.raises(ValueError, match="bvh"):
        E.MeshWinding(_mesh(v, f), D.LO, D.HI, bvh=wd.bvh)             # another mesh's tensors
    empty = E.MeshWinding(_mesh(v, np.zeros((0, 3), np.int32)), D.LO, D.HI)
    ew, ev = empty.query(tp)
    fin = np.isfinite(pts).all(1)
    assert empty.P == 1 and not empty.moments.any() and (ew.cpu().numpy()[fin] == 0.0).all() and not ev.any()
    assert np.isnan(ew.cpu().numpy()[~fin]).all()


def test_a_permuted_face_list():
    """The exact sum (beta = inf) under a permuted face list: the keys order faces of one Morton cell by their index, so the order
    of the sum may change, and nothing else: within F * 2^-48."""
    v, f, pts, _ = _case("sphere24")
    perm = np.random.default_rng(9).permutation(len(f))
    w0, v0 = _Wind(v, f).query(pts, np.inf)
    w1, v1 = _Wind(v, f[perm], BIG_BYTES).query(pts, np.inf)
    fin = np.isfinite(pts).all(1)
    assert np.array_equal(v0, v1) and np.abs(w0[fin] - w1[fin]).max() <= len(f) * CAP
    want = W.exact_sum(pts, v, f)
    assert np.abs(w0[fin] - want[fin]).max() <= len(f) * CAP


# ------------------------------------------------------------------------------------------------ volume, remesh, signed distance
@functools.lru_cache(maxsize=None)
def _open_cube_volume():
    vo, fo = W.open_cube()
    wd = W.Winding(vo, fo)
    vol, w64 = wd.volume(16, D.LO, D.HI, 2.0)
    return vo, fo, vol, w64


def test_volume_and_remesh_of_the_open_cube():
    from nerf_meets_mlx_amd.engine import mesh as E
    vo, fo, vol, w64 = _open_cube_volume()
    assert np.abs(w64 - 0.5).min() > 1e-6                              # the mirror's precondition: no lattice value on the level
    m = _mesh(vo, fo)
    got = E.winding_volume(m, 16, D.LO, D.HI)
    assert got.shape == (16, 16, 16) and got.dtype == torch.float32
    g = got.cpu().numpy().astype(np.float64)
    assert (np.abs(g - w64) <= len(fo) * CAP + np.abs(w64) * 2.0 ** -24).all()              # the cap and one float32 rounding
    assert np.array_equal((g > 0.5), (w64 > 0.5))
    mv, mf, _ = M.marching_cubes(vol, 0.5, D.LO, D.HI)
    r = E.remesh(m, 16, D.LO, D.HI)
    rv, rf = r.verts.cpu().numpy(), r.faces.cpu().numpy()
    assert r.colors is None and np.array_equal(rf, mf) and M.closed_and_oriented(rf) and (M.undirected_edge_counts(rf) == 2).all()
    assert np.abs(rv - mv).max() <= 1e-6 * (np.array(D.HI) - np.array(D.LO)).max()
    same = E.remesh(m, 16, D.LO, D.HI, min_component=2, largest_only=True)                             # one piece: kept
    assert torch.equal(same.faces, r.faces) and bits_equal(same.verts, r.verts)
    # the options reach the volume stage as they are: the opening takes the corner voxels off, as it does for a density volume
    opened = E.remesh(m, 16, D.LO, D.HI, min_component=2, largest_only=True, opening_radius=1)
    want = E.marching_cubes(E.filter_volume(got, 0.5, 2, True, 1), 0.5, D.LO, D.HI)
    assert torch.equal(opened.faces, want.faces) and bits_equal(opened.verts, want.verts)
    assert 0 < opened.faces.shape[0] != r.faces.shape[0] and M.closed_and_oriented(opened.faces.cpu().numpy())
    gone = E.remesh(m, 16, D.LO, D.HI, min_component=16 ** 3)                                          # nothing is that large
    assert gone.faces.shape == (0, 3) and gone.verts.shape == (0, 3)


def test_signed_distance_on_the_cube():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = D.cube()
    m = _mesh(v, f)
    named = np.array([[0.0, 0.75, 1.5], [0.75, 0.75, 1.5], [0.1, np.nan, 1.0]], np.float32)     # the centre, 0.25 outside x = 0.5, NaN
    pts = np.concatenate([named, D.query_points(v, f, 120, 7)])
    tp = _dev(pts, torch.float32)
    sd, face, w = E.signed_distance(tp, m, D.LO, D.HI)
    assert sd.dtype == torch.float32 and face.dtype == torch.int32 and w.dtype == torch.float64
    s = sd.cpu().numpy()
    assert s[0] == -0.5 and s[1] == 0.25 and np.isnan(s[2]) and np.isnan(w.cpu().numpy()[2])
    _, _, exact = E.signed_distance(tp, m, D.LO, D.HI, beta=float("inf"))
    assert abs(float(exact[0]) - 1.0) < 1e-12 and abs(float(exact[1])) < 1e-12
    d2, fc = E.MeshBVH(m, D.LO, D.HI).query(tp)
    assert torch.equal(face, fc) and bits_equal(sd.abs(), d2.double().sqrt().float())
    assert float(sd[0]) ** 2 == float(d2[0]) and float(sd[1]) ** 2 == float(d2[1])
    fin = np.isfinite(pts).all(1)
    assert np.array_equal(s[fin] < 0, w.cpu().numpy()[fin] > 0.5)
    off = np.abs(pts[fin] - v.mean(0)).max(1) != 0.5                   # off the surface, the sign is the cube's own
    assert np.array_equal((s[fin] < 0)[off], (np.abs(pts[fin] - v.mean(0)).max(1) < 0.5)[off])
    gs, gf, gw = E.signed_distance(tp, m, D.LO, D.HI, index="grid")
    assert bits_equal(gs, sd) and torch.equal(gf, face) and torch.equal(gw.view(torch.int64), w.view(torch.int64))
    with pytest.raises(ValueError, match="index"):
        E.signed_distance(tp, m, D.LO, D.HI, index="octree")
