"""Mesh smoothing on the GPU (csrc/smooth.hip, engine/mesh smooth, mesh_volume / Trainer.extract_mesh with smooth_iterations)
against the numpy reference of tests/_smooth_ref.py: vertex, normal and colour-row bits compared as integers -- no tolerance
anywhere, the rule is exact -- into sentinel-filled outputs with a poisoned workspace; both parities of the ping-pong with and
without the mu half-step; rows longer than a wave and than a workgroup; ignored faces, a NaN vertex, an unreferenced vertex;
reproducibility and a permuted face list; the C ABI's argument errors; the pipeline's order and its colour rows."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _mesh_ref as M
from tests import _smooth_ref as S
from tests._poison import BIG_BYTES, NAN_BYTES, bits_equal, poison_, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
E_NULL, E_SHAPE = -1, -2
SETTINGS = [(1, S.MU), (2, S.MU), (7, S.MU), (1, 0.0), (2, 0.0), (7, 0.0)]      # 2, 4, 14, 1, 2, 7 half-steps


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, order="C")).to(device=DEV, dtype=dtype).contiguous()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


class _Built:
    """nerf_smooth_build on numpy inputs with a poisoned workspace; run() are the other two C calls into sentinel outputs that
    carry one spare row each."""

    def __init__(self, v, f, pattern=NAN_BYTES, lo=S.LO, hi=S.HI):
        from nerf_meets_mlx_amd import _native as N
        self.N, self.L = N, N.lib()
        self.v0, self.f0 = np.array(v, np.float32).reshape(-1, 3), np.array(f, np.int32).reshape(-1, 3)
        self.tv, self.tf = _dev(self.v0, torch.float32), _dev(self.f0, torch.int32)
        self.V, self.F = self.tv.shape[0], self.tf.shape[0]
        self.lo, self.hi = (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)
        nbytes = self.L.nerf_smooth_workspace_bytes(self.V, self.F)
        assert nbytes > 0
        self.ws = poison_(torch.empty(nbytes, dtype=torch.uint8, device=DEV), pattern)
        N.check(self.L.nerf_smooth_build(self.V, N.ptr(self.tf), self.F, N.ptr(self.ws), N.stream()))

    def run(self, iterations, lam, mu, rows=True):
        N, L, V = self.N, self.L, self.V
        ov = sentinel_(torch.empty(V + 1, 3, dtype=torch.float32, device=DEV))
        on = sentinel_(torch.empty(V + 1, 3, dtype=torch.float32, device=DEV))
        orow = sentinel_(torch.empty(V + 1, 11, dtype=torch.float32, device=DEV)) if rows else None
        N.check(L.nerf_smooth_run(N.ptr(self.tv), V, self.lo, self.hi, iterations, lam, mu, N.ptr(self.ws), N.ptr(ov), N.stream()))
        N.check(L.nerf_smooth_normals(N.ptr(ov), V, self.lo, self.hi, N.ptr(self.ws), N.ptr(on), N.ptr(orow), N.stream()))
        torch.cuda.synchronize()
        assert unwritten(ov[V:]) == 3 and unwritten(on[V:]) == 3 and (orow is None or unwritten(orow[V:]) == 11)
        assert np.array_equal(_bits(self.tv.cpu().numpy()), _bits(self.v0)) and np.array_equal(self.tf.cpu().numpy(), self.f0)
        return ov[:V].cpu().numpy(), on[:V].cpu().numpy(), None if orow is None else orow[:V].cpu().numpy()


def _assert_same(got, want, what=""):
    gv, gn, rows = got
    wv, wn = want
    dv = (_bits(gv) != _bits(wv)).any(1)
    assert not dv.any(), (what, "vertex bits differ", int(dv.sum()), np.nonzero(dv)[0][:4], gv[dv][:4], wv[dv][:4])
    dn = (_bits(gn) != _bits(wn)).any(1)
    assert not dn.any(), (what, "normal bits differ", int(dn.sum()), np.nonzero(dn)[0][:4], gn[dn][:4], wn[dn][:4])
    if rows is not None:
        assert np.array_equal(_bits(rows), _bits(S.color_rows(wv, wn))), (what, "colour rows differ")


def _mesh(name):
    if name == "junk":
        return S.junk(12)[:2]
    return {"tetrahedron": S.tetrahedron, "sphere12": lambda: S.sphere(12), "sphere24": lambda: S.sphere(24), "strip": S.strip,
            "fan300": lambda: S.fan(300), "fan256": lambda: S.fan(256)}[name]()


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name,V", [("tetrahedron", 4), ("sphere12", 386), ("sphere24", 2074), ("strip", 42), ("fan300", 301),
                                    ("fan256", 257), ("junk", 387)])
def test_smooth_matches_the_reference_bit_for_bit(name, V):
    v, f = _mesh(name)
    assert len(v) == V
    built = _Built(v, f)
    for iterations, mu in SETTINGS:
        want = S.smooth(v, f, iterations, S.LO, S.HI, S.LAM, mu)
        _assert_same(built.run(iterations, S.LAM, mu), want, (name, iterations, mu))
    if name == "junk":                                               # the NaN vertex and the unreferenced one: copied, normal 0
        gv, gn, _ = built.run(2, S.LAM, S.MU)
        _, _, i_nan, i_free = S.junk(12)
        assert np.array_equal(_bits(gv[[i_nan, i_free]]), _bits(np.asarray(v)[[i_nan, i_free]])) and not gn[[i_nan, i_free]].any()
        assert np.isfinite(np.delete(gv, i_nan, 0)).all()


def test_an_odd_box_other_factors_and_special_values():
    """A box that is no cube and whose extents are no binary fractions, lambda 1 and mu -2 (the range's ends), infinities."""
    v, f = (a.copy() for a in S.sphere(12))
    v[5, 0], v[40, 2], v[41] = np.inf, -np.inf, [9.0, -7.0, 30.0]      # (41: far outside the box, inside the clamp)
    lo, hi = [-1.7, -0.9, 0.3], [1.3, 2.9, 3.0]
    built = _Built(v, f, BIG_BYTES, lo, hi)
    for iterations, lam, mu in ((3, 1.0, -2.0), (2, 0.3, -0.31), (1, 1.0, 0.0)):
        _assert_same(built.run(iterations, lam, mu), S.smooth(v, f, iterations, lo, hi, lam, mu), (iterations, lam, mu))


# ------------------------------------------------------------------------------------------------ reproducibility
def test_two_runs_two_workspaces_and_a_permuted_face_list_give_the_same_bits():
    v, f = S.sphere(24)
    a = _Built(v, f, NAN_BYTES)
    first, again = a.run(7, S.LAM, S.MU), a.run(7, S.LAM, S.MU)
    other = _Built(v, f, BIG_BYTES).run(7, S.LAM, S.MU)
    perm = _Built(v, f[np.random.default_rng(11).permutation(len(f))]).run(7, S.LAM, S.MU)
    for b in (again, other, perm):
        for x, y in zip(first, b):
            assert np.array_equal(_bits(x), _bits(y))
    assert a.run(7, S.LAM, S.MU, rows=False)[2] is None                 # color_rows NULL: the other outputs are checked in run()


def test_empty_meshes():
    from nerf_meets_mlx_amd.engine import mesh as E
    z3, zf = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    v, _ = S.tetrahedron()
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    assert L.nerf_smooth_workspace_bytes(0, 0) >= 0
    assert L.nerf_smooth_build(0, None, 0, None, N.stream()) == 0
    gv, gn, rows = _Built(v, zf).run(3, S.LAM, S.MU)                   # no face: every vertex is copied, every normal 0
    assert np.array_equal(_bits(gv), _bits(v)) and not gn.any() and np.array_equal(_bits(rows[:, :3]), _bits(v))
    for vv in (z3, v):
        m = E.smooth(E.Mesh(_dev(vv, torch.float32).reshape(-1, 3), _dev(zf, torch.int32).reshape(-1, 3),
                            _dev(vv, torch.float32).reshape(-1, 3)), 2, S.LO, S.HI)
        assert m.verts.shape == (len(vv), 3) and m.faces.shape == (0, 3) and bits_equal(m.verts.cpu(), torch.from_numpy(vv))


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_return_before_any_device_work():
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    v, f = S.sphere(12)
    tv, tf = _dev(v, torch.float32), _dev(f, torch.int32)
    V, F = len(v), len(f)
    lo, hi = (C.c_float * 3)(*S.LO), (C.c_float * 3)(*S.HI)
    flat = (C.c_float * 3)(1.5, -0.7, 3.1)                              # hi_y = lo_y
    nanbox = (C.c_float * 3)(float("nan"), 2.3, 3.1)
    ws = poison_(torch.empty(L.nerf_smooth_workspace_bytes(V, F), dtype=torch.uint8, device=DEV), NAN_BYTES)
    ov = sentinel_(torch.empty(V, 3, dtype=torch.float32, device=DEV))
    on = sentinel_(torch.empty(V, 3, dtype=torch.float32, device=DEV))
    rows = sentinel_(torch.empty(V, 11, dtype=torch.float32, device=DEV))
    st = N.stream()
    big = (1 << 24) + 1
    nan = float("nan")

    def build(V=V, faces=tf, F=F, ws=ws):
        return L.nerf_smooth_build(V, N.ptr(faces), F, N.ptr(ws), st)

    def run(verts=tv, V=V, lo=lo, hi=hi, it=3, lam=0.5, mu=-0.53, ws=ws, out=ov):
        return L.nerf_smooth_run(N.ptr(verts), V, lo, hi, it, lam, mu, N.ptr(ws), N.ptr(out), st)

    def normals(verts=tv, V=V, lo=lo, hi=hi, ws=ws, out=on, rows=rows):
        return L.nerf_smooth_normals(N.ptr(verts), V, lo, hi, N.ptr(ws), N.ptr(out), N.ptr(rows), st)

    for kw in ({"V": big}, {"V": -1}, {"F": big}, {"F": -1}):
        assert build(**kw) == E_SHAPE, kw
        assert b"nerf_smooth_build" in L.nerf_last_error()
    for kw in ({"lam": 0.0}, {"lam": nan}, {"lam": -0.5}, {"lam": 1.5}, {"mu": 0.25}, {"mu": nan}, {"mu": -2.5}, {"it": 0},
               {"it": 1025}, {"it": -3}, {"hi": flat}, {"hi": lo}, {"lo": nanbox}, {"V": big}, {"V": -1}):
        assert run(**kw) == E_SHAPE, kw
        assert b"nerf_smooth_run" in L.nerf_last_error()
    for kw in ({"hi": flat}, {"lo": nanbox}, {"V": big}, {"V": -1}):
        assert normals(**kw) == E_SHAPE, kw
        assert b"nerf_smooth_normals" in L.nerf_last_error()
    for kw in ({"faces": None}, {"ws": None}):
        assert build(**kw) == E_NULL, kw
    for kw in ({"verts": None}, {"ws": None}, {"out": None}, {"lo": None}, {"hi": None}):
        assert run(**kw) == E_NULL, kw
    for kw in ({"verts": None}, {"ws": None}, {"out": None}, {"lo": None}):
        assert normals(**kw) == E_NULL, kw
    assert b"nerf_smooth_normals" in L.nerf_last_error()
    for bad in ((-1, 0), (0, -1), (big, 0), (0, big)):
        assert L.nerf_smooth_workspace_bytes(*bad) == -1
    torch.cuda.synchronize()
    assert unwritten(ov) == ov.numel() and unwritten(on) == on.numel() and unwritten(rows) == rows.numel()
    assert bool((ws == NAN_BYTES).all())
    assert np.array_equal(_bits(tv.cpu().numpy()), _bits(v)) and np.array_equal(tf.cpu().numpy(), f)


# ------------------------------------------------------------------------------------------------ engine and pipeline
R_PIPE, ISO = 16, 0.0


@pytest.fixture(scope="module")
def volume():
    """The noisy sphere's volume at R = 16 on the device, and a query that records the rows it is asked and answers a fixed
    function of them."""
    p = M.lattice_points(R_PIPE, S.LO, S.HI).astype(np.float64)
    noise = np.random.default_rng(R_PIPE).standard_normal(R_PIPE ** 3)
    vol = (S.RADIUS - np.linalg.norm(p - S.CENTRE, axis=1) + S.NOISE * noise).reshape((R_PIPE,) * 3).astype(np.float32)
    seen = []

    def query(rows, z):
        seen.append(rows.clone())
        raw = torch.zeros(rows.shape[0], 1, 4, dtype=torch.float32, device=rows.device)
        raw[:, 0, :3] = 0.5 + 0.6 * torch.sin(3.0 * rows[:, :3] + rows[:, 3:6])
        return raw

    return _dev(vol, torch.float32), vol, query, seen


def _rows_of(m):
    rows = torch.zeros(m.verts.shape[0], 11, dtype=torch.float32, device=m.verts.device)
    rows[:, 0:3], rows[:, 3:6], rows[:, 8:11] = m.verts, -m.normals, -m.normals
    return rows


def _same_mesh(a, b):
    return bits_equal(a.verts, b.verts) and torch.equal(a.faces, b.faces) and bits_equal(a.normals, b.normals) \
        and ((a.colors is None and b.colors is None) or bits_equal(a.colors, b.colors))


def test_engine_smooth_matches_the_reference_and_carries_faces_and_colors(volume):
    from nerf_meets_mlx_amd.engine import mesh as E
    tvol, vol, _, _ = volume
    raw = E.marching_cubes(tvol, ISO, S.LO, S.HI)
    col = torch.rand(raw.verts.shape[0], 3, device=DEV)
    before = raw.verts.clone()
    m = E.smooth(raw._replace(colors=col), 3, S.LO, S.HI)
    assert m.faces is raw.faces and m.colors is col and bits_equal(raw.verts, before)
    want = S.smooth(raw.verts.cpu().numpy(), raw.faces.cpu().numpy(), 3, S.LO, S.HI)
    assert np.array_equal(_bits(m.verts.cpu().numpy()), _bits(want[0])) and np.array_equal(_bits(m.normals.cpu().numpy()), _bits(want[1]))
    lap = E.smooth(raw, 3, S.LO, S.HI, lam=0.5, mu=0.0)
    want = S.smooth(raw.verts.cpu().numpy(), raw.faces.cpu().numpy(), 3, S.LO, S.HI, 0.5, 0.0)
    assert lap.colors is None and np.array_equal(_bits(lap.verts.cpu().numpy()), _bits(want[0]))
    for bad in ({"iterations": 0}, {"iterations": 1025}, {"iterations": 2, "lam": 0.0}, {"iterations": 2, "mu": 0.5}):
        with pytest.raises(ValueError):
            E.smooth(raw, lo=S.LO, hi=S.HI, **bad)


def test_mesh_volume_smooths_between_marching_cubes_and_the_simplifier(volume):
    from nerf_meets_mlx_amd.engine import mesh as E
    tvol, _, query, seen = volume
    raw = E.marching_cubes(tvol, ISO, S.LO, S.HI)
    assert raw.verts.shape[0] > 300
    by_hand = E.smooth(raw, 3, S.LO, S.HI)
    # smoothing alone: the colour query sees the smoother's rows
    del seen[:]
    got = E.mesh_volume(query, tvol, ISO, S.LO, S.HI, True, smooth_iterations=3)
    assert _same_mesh(got._replace(colors=None), by_hand) and torch.equal(got.faces, raw.faces)
    assert len(seen) == 1 and bits_equal(seen[0], _rows_of(by_hand))
    assert bits_equal(got.colors, E.vertex_colors(query, _rows_of(by_hand)))
    assert _same_mesh(E.mesh_volume(query, tvol, ISO, S.LO, S.HI, False, smooth_iterations=3), by_hand)
    # with the simplifier behind it: the query sees the simplified mesh's rows
    simp = E.simplify(by_hand, 8, S.LO, S.HI)
    assert 0 < simp.verts.shape[0] < raw.verts.shape[0]
    del seen[:]
    got = E.mesh_volume(query, tvol, ISO, S.LO, S.HI, True, simplify_grid=8, smooth_iterations=3)
    assert _same_mesh(got._replace(colors=None), simp)
    assert len(seen) == 1 and bits_equal(seen[0], _rows_of(simp))
    # other factors reach the kernel
    lap = E.mesh_volume(query, tvol, ISO, S.LO, S.HI, False, smooth_iterations=3, smooth_lambda=0.4, smooth_mu=0.0)
    assert _same_mesh(lap, E.smooth(raw, 3, S.LO, S.HI, 0.4, 0.0)) and not bits_equal(lap.verts, by_hand.verts)
    # 0 is the parent's path, bit for bit, with the same single query on marching cubes' own rows
    del seen[:]
    a = E.mesh_volume(query, tvol, ISO, S.LO, S.HI, True)
    b = E.mesh_volume(query, tvol, ISO, S.LO, S.HI, True, smooth_iterations=0)
    assert _same_mesh(a, b) and len(seen) == 2 and bits_equal(seen[0], seen[1]) and bits_equal(a.verts, raw.verts)
    assert bits_equal(seen[0], _rows_of(raw))
    for bad in ({"smooth_iterations": -1}, {"smooth_iterations": 1025}, {"smooth_iterations": 2.0}, {"smooth_iterations": True},
                {"smooth_iterations": 2, "smooth_lambda": 0.0}, {"smooth_iterations": 2, "smooth_mu": 0.3}):
        with pytest.raises(ValueError):
            E.mesh_volume(query, tvol, ISO, S.LO, S.HI, False, **bad)


def test_trainer_extract_mesh_with_smooth_iterations():
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine import mesh as E
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    imgs, poses, _, _, K = synthetic.make_dataset(8, 8, 2, seed=0, device=DEV)
    tr = Trainer(imgs, poses, K, N_rand=64, n_depth_samples=16, N_importance=16, seed=4, device=DEV)
    box = ([-1.0] * 3, [1.0] * 3)
    vol = tr.density_volume(16, box)
    thr = float(vol.reshape(-1).quantile(0.7))
    print("untrained field: density min / threshold / max", float(vol.min()), thr, float(vol.max()))
    assert float(vol.min()) < thr < float(vol.max())
    raw = tr.extract_mesh(resolution=16, threshold=thr, aabb=box)
    s = tr.extract_mesh(resolution=16, threshold=thr, aabb=box, smooth_iterations=2)
    print("V, F", raw.verts.shape[0], raw.faces.shape[0])
    assert raw.faces.shape[0] > 0 and torch.equal(s.faces, raw.faces)
    want = E.smooth(raw._replace(colors=None), 2, *box)
    assert bits_equal(s.verts, want.verts) and bits_equal(s.normals, want.normals) and not bits_equal(s.verts, raw.verts)
    assert s.colors.shape == raw.colors.shape and bits_equal(s.colors, E.vertex_colors(tr._mesh_field()[0], _rows_of(s)))
    assert _same_mesh(raw, tr.extract_mesh(resolution=16, threshold=thr, aabb=box, smooth_iterations=0))
    with pytest.raises(ValueError):
        tr.extract_mesh(resolution=16, threshold=thr, aabb=box, smooth_iterations=2, smooth_mu=1.0)
