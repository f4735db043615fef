"""Mesh distance without a GPU: the numpy mirror (tests/_distance_ref.py) of include/nerf_hip.h "mesh distance" held to a float64
closed form and to the binomial law, the argument checks of engine.mesh and of the C entries (all of them return before any
device work), and the header / binding / Makefile bookkeeping.  The GPU side is held to the mirror bit for bit in
tests/test_gpu_distance.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _distance_ref as D
from tests import _smooth_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE = -1, -2
ENTRIES = ["nerf_meshdist_build", "nerf_meshdist_count", "nerf_meshdist_query", "nerf_meshdist_workspace_bytes", "nerf_surface_cdf",
           "nerf_surface_cdf_workspace_bytes", "nerf_surface_sample"]


# ------------------------------------------------------------------------------------------------ the point-triangle mirror
A, B, CC = np.array([1.0, 2.0, 0.5]), np.array([4.0, 2.0, 0.5]), np.array([1.0, 6.0, 0.5])     # right angle at A, legs 3 and 4, z = 0.5
REGION_POINTS = {"vertex a": ([0.0, 1.5, 1.0], A), "vertex b": ([5.5, 1.0, 0.0], B), "vertex c": ([0.5, 7.5, 1.5], CC),
                 "edge ab": ([2.5, 0.5, 1.25], [2.5, 2.0, 0.5]), "edge ac": ([-1.0, 4.0, 0.0], [1.0, 4.0, 0.5]),
                 "edge bc": ([4.5, 5.5, 0.5], [2.5, 4.0, 0.5]), "interior": ([1.75, 3.0, 2.5], [1.75, 3.0, 0.5])}


def _closest_f64(p, a, b, c):
    """The closest point of the triangle by a closed form that shares nothing with Ericson's tests: the minimum over the three
    segments and, where the foot of the perpendicular has barycentrics in [0, 1], the foot."""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    cand = []
    for u, v in ((a, b), (a, c), (b, c)):
        t = np.clip(np.dot(p - u, v - u) / np.dot(v - u, v - u), 0.0, 1.0)
        cand.append(u + t * (v - u))
    n = np.cross(b - a, c - a)
    foot = p - n * (np.dot(p - a, n) / np.dot(n, n))
    M = np.stack([b - a, c - a], 1)
    s, t = np.linalg.lstsq(M, foot - a, rcond=None)[0]
    if s >= 0 and t >= 0 and s + t <= 1:
        cand.append(foot)
    return min(float(np.dot(p - q, p - q)) for q in cand)


@pytest.mark.parametrize("region", sorted(REGION_POINTS))
def test_the_mirror_agrees_with_a_float64_closed_form_in_every_region(region):
    """Every input here is exact in float32.  The mirror reaches p - q in at most ten float32 operations (a subtraction, a dot
    product, a quotient, a product and a sum per coordinate of q, then the difference) on operands of magnitude at most S = 8,
    the squares in the dot products at most 4 S^2: each rounds by at most 2^-24 of its result, so q is off by at most
    10 * 2^-24 * 4 S per coordinate, generously, and |p - q|^2 by 2 |p - q| sqrt(3) times that plus three roundings of the sum.
    With |p - q| <= 4: 2 * 4 * 1.74 * 10 * 2^-24 * 32 + 3 * 2^-24 * 16 < 4600 * 2^-24 = 2.8e-4 absolute; the observed error is
    far inside it, the bound is what the operation count allows."""
    p, q = REGION_POINTS[region]
    want = _closest_f64(p, A, B, CC)
    if q is not None:
        assert abs(want - float(np.sum((np.array(p) - np.array(q)) ** 2))) < 1e-12      # the closed form lands where it should
    got = float(D.point_triangle_d2(np.array(p, np.float32), A.astype(np.float32), B.astype(np.float32), CC.astype(np.float32)))
    assert want > 0.25 and abs(got - want) <= 4600 * 2.0 ** -24, (region, got, want)
    for a, b, c in ((B, CC, A), (CC, A, B), (A, CC, B)):                                  # the rule does not depend on the corner order
        again = float(D.point_triangle_d2(np.array(p, np.float32), a.astype(np.float32), b.astype(np.float32), c.astype(np.float32)))
        assert abs(again - want) <= 4600 * 2.0 ** -24


def test_the_three_corners_are_at_exactly_zero():
    for v, f in (((A, B, CC), None), S.tetrahedron(), D.cube()):
        if f is None:
            tri = [np.array(v, np.float32)]
        else:
            tri = [v[face] for face in f]
        for t in tri:
            for k in range(3):
                d = D.point_triangle_d2(t[k], t[0], t[1], t[2])
                assert d.view(np.uint32) == 0, (t, k, d)


def test_brute_force_takes_the_lowest_face_on_a_tie_and_skips_invalid_faces():
    v, f = D.junk()
    ok, a, b, c, _ = D.corners(v, f)
    assert (~ok).sum() >= 8 + 2 + 3                           # bad indices and equal corners, two degenerate, around the NaN vertex
    fin = np.isfinite(v).all(1)
    pts = np.concatenate([v[fin][:60], ((a[ok] + b[ok]) * np.float32(0.5))[:20]])
    d2, face = D.brute_force(pts, v, f)
    assert (d2 < 1e-10).all() and ok[face].all()
    ties = 0
    for p, dd, fc in zip(pts, d2, face):                      # one point against every valid face, then numpy's first minimum
        every = D.point_triangle_d2(p, a[ok], b[ok], c[ok])
        assert dd == every.min() and fc == np.nonzero(ok)[0][np.argmin(every)]
        ties += int((every == every.min()).sum() > 1)
    assert ties >= 40                                         # vertices and edge midpoints are shared
    d2, face = D.brute_force(np.array([[np.nan, 0, 0], [0.0, 0.0, np.inf]], np.float32), v, f)
    assert np.isnan(d2).all() and (face == -1).all()
    d2, face = D.brute_force(v[:3], v, f[~ok])
    assert np.isposinf(d2).all() and (face == -1).all()


# ------------------------------------------------------------------------------------------------ the sampler mirror
def _two_faces():
    """Areas 1 : 3 (doubled areas 1 and 3, exact), plus a zero-area face and a face with a bad index."""
    v = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1], [0, 0, 2], [3, 0, 2], [0, 1, 2], [0.5, 0.5, 1.0]], np.float32)
    f = np.array([[0, 1, 2], [0, 6, 6], [3, 4, 5], [0, 1, 7], [0, 0, 1]], np.int32)
    return v, f


def test_sampler_follows_the_areas_within_five_binomial_deviations():
    """n = 4096 draws with p = 1/4: the smaller face's count has mean 1024 and deviation sqrt(4096 * 1/4 * 3/4) = 27.7; five of
    them are 138.6, so the count lies within 139 of 1024 unless the draws are not independent and uniform (a 1.2e-6 event)."""
    v, f = _two_faces()
    w = D.weights(v, f, S.LO, S.HI)
    assert w[0] > 2 ** 30 and abs(int(w[2]) - 3 * int(w[0])) <= 2 and not w[[1, 3, 4]].any()   # 1 : 3 up to the rounding to units
    for seed in (0, 7):
        pts, face, u = D.sample(v, f, 4096, S.LO, S.HI, seed)
        assert set(np.unique(face)) == {0, 2}                                            # invalid faces are never drawn
        assert abs(int((face == 0).sum()) - 1024) <= 139, (seed, int((face == 0).sum()))
        u = u.astype(np.float64)
        assert (u >= 0).all() and (u <= 1).all() and (u.sum(1) <= 1.0).all()             # barycentrics (1 - u1 - u2, u1, u2)
        assert (pts[face == 0][:, 2] == 1).all() and (pts[face == 2][:, 2] == 2).all()
        lo = np.where(face == 0, 0.0, 0.0)
        assert (pts[:, 0] >= lo).all() and (pts[:, 1] >= 0).all()
        assert (pts[face == 0][:, :2].sum(1) <= 1.0 + 1e-6).all() and (pts[face == 2][:, 0] / 3 + pts[face == 2][:, 1] <= 1.0 + 1e-6).all()
    a, _, _ = D.sample(v, f, 10, S.LO, S.HI, 3)
    b, _, _ = D.sample(v, f, 300, S.LO, S.HI, 3)
    assert np.array_equal(a, b[:10])                                                       # sample i depends on (seed, i) alone
    with pytest.raises(ValueError):
        D.sample(v, f[[1, 3, 4]], 5, S.LO, S.HI)


def test_weights_are_exact_integers_with_the_stated_bounds():
    assert 2 ** 24 * D.W_LIM * D.W_SCALE < 2 ** 63 and 512.0 ** -2 * D.W_SCALE >= 2 ** 16
    v, f = S.sphere(12)
    w = D.weights(v, f, S.LO, S.HI)
    perm = np.random.default_rng(0).permutation(len(f))
    assert w.dtype == np.int64 and (w > 0).all() and D.cdf(v, f[perm], S.LO, S.HI)[-1] == w.sum()
    area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]].astype(np.float64) - v[f[:, 0]], v[f[:, 2]].astype(np.float64) - v[f[:, 0]]), axis=1)
    assert np.allclose(w / w.sum(), area / area.sum(), rtol=1e-4)
    assert [D.default_grid(F) for F in (0, 4, 31, 32, 768, 4064, 692000, 1 << 24)] == [1, 1, 1, 1, 4, 11, 147, 256]


# ------------------------------------------------------------------------------------------------ host-side API
def test_argument_checks():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = (torch.from_numpy(a.copy()) for a in S.sphere(12))
    n = torch.zeros_like(v)
    good = E.Mesh(v, f, n, None)
    pts = torch.zeros(5, 3)
    assert E.check_distance_args(good, 5, S.LO, S.HI) == (5, S.LO, S.HI, None, 0, None)
    assert E.check_distance_args(good, np.int64(5), S.LO, S.HI, 1, 2 ** 64 - 1, 0.5, pts) == (5, S.LO, S.HI, 1, 2 ** 64 - 1, 0.5)
    assert E.check_distance_args(good, 0, S.LO, S.HI, E.DISTANCE_MAX_GRID, 7, np.float32(0.25))[3:] == (256, 7, 0.25)
    for bad in (-1, (1 << 30) + 1, 3.0, True, None, "3"):
        with pytest.raises(ValueError):
            E.check_distance_args(good, bad, S.LO, S.HI)
    for bad in (0, -1, 257, 2.0, True, "4"):
        with pytest.raises(ValueError):
            E.check_distance_args(good, 5, S.LO, S.HI, bad)
    for bad in (-1, 2 ** 64, 1.0, False, None, "0"):
        with pytest.raises(ValueError):
            E.check_distance_args(good, 5, S.LO, S.HI, None, bad)
    for bad in (0.0, -0.5, float("nan"), float("inf"), True, "0.1"):
        with pytest.raises(ValueError):
            E.check_distance_args(good, 5, S.LO, S.HI, None, 0, bad)
    for lo, hi in (([0.0] * 3, [0.0] * 3), ([-1, -1, 1], [1, 1, 1]), ([-1, -1], [1, 1]), ([-1, -1, float("nan")], [1, 1, 1])):
        with pytest.raises(ValueError):
            E.check_distance_args(good, 5, lo, hi)
    for m in (good._replace(verts=v.double()), good._replace(faces=f.long()), good._replace(normals=n[:-1]), (v, f), None):
        with pytest.raises(ValueError):
            E.check_distance_args(m, 5, S.LO, S.HI)
    for p in (pts.double(), pts[:4], pts.t().contiguous().t(), pts[:, :2], pts.numpy(), torch.zeros(5, 3, device="meta")):
        with pytest.raises(ValueError):
            E.check_distance_args(good, 5, S.LO, S.HI, points=p)
    with pytest.raises(ValueError):
        E.mesh_distance(good, good, 0, S.LO, S.HI)
    assert [E.default_distance_grid(F) for F in (0, 4, 768, 4064, 692000, 1 << 24)] == [D.default_grid(F) for F in (0, 4, 768, 4064, 692000, 1 << 24)]


def test_trainers_offer_mesh_distance():
    import inspect
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    for cls in (Trainer, NGPTrainer):
        p = inspect.signature(cls.mesh_distance).parameters
        assert list(p) == ["self", "mesh", "other", "n", "tau", "seed", "aabb"]
        assert (p["n"].default, p["tau"].default, p["seed"].default, p["aabb"].default) == (1 << 20, None, 0, None)
    assert NGPTrainer.mesh_distance is Trainer.mesh_distance and NGPTrainer._mesh_box is not Trainer._mesh_box


def test_mesh_tool_has_the_distance_arm():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ngp_mesh_tool", os.path.join(ROOT, "tools", "ngp_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parser().parse_args(["--distance", "--distance-n", "4096"])
    assert a.distance and a.distance_n == 4096
    d = tool.parser().parse_args([])
    assert not d.distance and d.distance_n == 1 << 20
    assert callable(tool.near_union_boundary) and callable(tool._distance_arms)


def test_c_entries_refuse_before_any_device_work():
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    lo, hi = (C.c_float * 3)(*S.LO), (C.c_float * 3)(*S.HI)
    flat, nanbox = (C.c_float * 3)(1.5, -0.7, 3.1), (C.c_float * 3)(float("nan"), 2.3, 3.1)
    p = C.c_void_p(4096)                                               # never dereferenced: every call below is refused
    big = (1 << 24) + 1

    def cdf(verts=p, V=4, faces=p, F=4, lo=lo, hi=hi, ws=p, out=p):
        return L.nerf_surface_cdf(verts, V, faces, F, lo, hi, ws, out, None)

    def sample(verts=p, V=4, faces=p, F=4, cdf=p, total=10, n=5, pts=p, face=p):
        return L.nerf_surface_sample(verts, V, faces, F, cdf, total, n, 0, pts, face, None)

    def count(verts=p, V=4, faces=p, F=4, lo=lo, hi=hi, G=4, ws=p, tot=p):
        return L.nerf_meshdist_count(verts, V, faces, F, lo, hi, G, ws, tot, None)

    def build(verts=p, V=4, faces=p, F=4, lo=lo, hi=hi, G=4, ws=p, ent=p, E=9):
        return L.nerf_meshdist_build(verts, V, faces, F, lo, hi, G, ws, ent, E, None)

    def query(pts=p, n=5, verts=p, V=4, faces=p, F=4, lo=lo, hi=hi, G=4, ws=p, ent=p, E=9, d=p, face=p):
        return L.nerf_meshdist_query(pts, n, verts, V, faces, F, lo, hi, G, ws, ent, E, d, face, None)

    shape = [{"V": big}, {"V": -1}, {"F": big}, {"F": -1}, {"hi": flat}, {"hi": lo}, {"lo": nanbox}]
    for fn, name, more in ((cdf, b"nerf_surface_cdf", []), (count, b"nerf_meshdist_count", [{"G": 0}, {"G": 257}, {"G": -3}]),
                           (build, b"nerf_meshdist_build", [{"G": 0}, {"G": 257}, {"E": -1}, {"E": (1 << 30) + 1}]),
                           (query, b"nerf_meshdist_query", [{"G": 0}, {"G": 257}, {"n": -1}, {"n": (1 << 30) + 1}, {"E": -1}])):
        for kw in shape + more:
            assert fn(**kw) == E_SHAPE, (name, kw)
            assert name in L.nerf_last_error()
    assert build(E=(1 << 30) + 1) == E_SHAPE and b"use a coarser grid" in L.nerf_last_error()
    for kw in ({"V": big}, {"F": -1}, {"n": -1}, {"n": (1 << 30) + 1}, {"total": 0}, {"total": -5}, {"F": 0}):
        assert sample(**kw) == E_SHAPE, kw
    assert sample(total=0) == E_SHAPE and b"no area" in L.nerf_last_error()
    for fn, kws in ((cdf, [{"faces": None}, {"ws": None}, {"out": None}, {"verts": None}, {"lo": None}, {"hi": None}]),
                    (sample, [{"verts": None}, {"faces": None}, {"cdf": None}, {"pts": None}, {"face": None}]),
                    (count, [{"verts": None}, {"faces": None}, {"ws": None}, {"tot": None}, {"lo": None}]),
                    (build, [{"verts": None}, {"faces": None}, {"ws": None}, {"ent": None}, {"hi": None}]),
                    (query, [{"pts": None}, {"verts": None}, {"faces": None}, {"ws": None}, {"ent": None}, {"d": None}, {"face": None},
                             {"lo": None}])):
        for kw in kws:
            assert fn(**kw) == E_NULL, (fn.__name__, kw)
    # nothing to do is no error, whatever the pointers
    assert sample(n=0, pts=None, face=None, total=0) == 0 and query(n=0, pts=None, d=None, face=None) == 0
    assert cdf(F=0, faces=None, ws=None, out=None) == 0 and build(E=0, ent=None) == 0
    for bad in ((-1, 4), (big, 4), (4, 0), (4, 257), (4, -1)):
        assert L.nerf_meshdist_workspace_bytes(*bad) == -1
    assert L.nerf_meshdist_workspace_bytes(0, 1) > 0
    assert L.nerf_meshdist_workspace_bytes(1 << 24, 256) == 8 * (1 << 16) + 16 + 4 * ((1 << 24) + 1) + 4 + 4 * (1 << 24)
    assert L.nerf_surface_cdf_workspace_bytes(-1) == -1 and L.nerf_surface_cdf_workspace_bytes(big) == -1
    assert L.nerf_surface_cdf_workspace_bytes(257) == 8 * 3


def test_header_section_bindings_and_makefile():
    from nerf_meets_mlx_amd import _native
    from nerf_meets_mlx_amd.engine import mesh as E
    text = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    start = text.index("mesh distance (no reference counterpart)")
    section = text[start:text.index("/* ----", start)]
    decl = re.sub(r"/\*.*?\*/", "", "/*" + section, flags=re.S)
    assert sorted(set(re.findall(r"\b(nerf_[a-z_]+)\s*\(", decl))) == ENTRIES
    lib = _native.lib()
    for e in ENTRIES:
        assert e in _native.SIGNATURES and hasattr(lib, e)
    assert lib.nerf_abi_version() == 3 and "#define NERF_ABI_VERSION 3" in text
    for word in ("max(1, (int64)rint(x * 2^34))", "Ericson", "0x632BE59BD9B4E019", "use a coarser grid", "Not done", "no BVH",
                 "no signed distance", "point-cloud-to-point-cloud"):
        assert word in section, word
    mk = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "Makefile")).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert "distance.hip" in srcs.split()
    assert not re.search(r"FLAGS_distance", mk)                                          # the default flags, -ffp-contract=off among them
    src = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "distance.hip")).read()
    kernels = sorted(set(re.findall(r"\b(\w+_kernel)\(", src)))
    assert kernels == ["dist_cdf_kernel", "dist_count_kernel", "dist_fill_kernel", "dist_query_kernel", "dist_sample_kernel",
                       "dist_weight_kernel"]
    # the cell offsets are csrc/scan.h's counts-to-offsets pair, defined there once and launched here: eight kernels as before
    scan = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "scan.h")).read()
    for name in ("scan_offsets_count_kernel", "scan_offsets_write_kernel"):
        assert len(re.findall(r"\b" + name + r"\(", scan)) == 1 and src.count(name + "<DIST_BLOCK>,") == 1, name
    assert "atomicAdd(float" not in src and not re.search(r"atomic\w*\(\s*\(float", src)
    for name in ("sample_surface", "MeshIndex", "point_mesh_distance", "mesh_distance", "MeshDistance", "check_distance_args"):
        assert hasattr(E, name) and name in open(os.path.join(ROOT, "nerf_meets_mlx_amd", "engine", "mesh", "distance.py")).read()
    assert "distance (sample_surface, MeshIndex, mesh_distance)" in E.__doc__
