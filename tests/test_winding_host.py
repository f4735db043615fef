"""The mesh winding number without a GPU: the numpy mirror (tests/_winding_ref.py) of include/nerf_hip.h "mesh winding number" held
to known values, its walk held to the sum in face order, the root moments, the dipole's error and its cost on sphere24, the open
cube closed by marching cubes of the mirror's volume, the workspace carve of csrc/winding_ws.h in a stand-alone program built with
the host compiler and -fsanitize=address,undefined (tests/winding_ws_check.cpp), the argument checks of engine.mesh and of the C
entries (all of them return before any device work), and the header / binding / Makefile bookkeeping.  The GPU side is held to the
mirror in tests/test_gpu_winding.py."""
import ctypes as C
import functools
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import _bvh_ref as B
from tests import _distance_ref as D
from tests import _mesh_ref as M
from tests import _smooth_ref as S
from tests import _winding_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE = -1, -2
ENTRIES = ["nerf_winding_build", "nerf_winding_query", "nerf_winding_workspace_bytes"]
# The mirror's own count on sphere24 (F = 4064, 1016 leaves) with D.query_points(.., 300, 5) at beta = 2: 257.61 faces evaluated
# per finite point (64.4 leaves entered) and 88.6 nodes approximated.  The cap is twice that: a walk that never approximated
# would evaluate all 4064.
SPHERE24_MEAN_FACES, SPHERE24_CAP = 257.61, 515.22
# The worst |w_beta - w_exact| over those points, measured on the mirror: 0.0143 at beta = 2 (0.0053 at 3).  The bar is twice it.
SPHERE24_DIPOLE_ERR, SPHERE24_DIPOLE_BAR = 0.0143, 0.03
CUBE_CENTRE = np.array([[0.0, 0.75, 1.5]], np.float32)


@functools.lru_cache(maxsize=None)
def _sphere24():
    """(verts, faces, the mirror, points, the face-order sum): computed once, shared, read-only."""
    v, f = D.MESHES["sphere24"]()
    pts = D.query_points(v, f, 300, 5)
    wd = W.Winding(v, f)
    exact = W.exact_sum(pts, v, f)
    for a in (pts, exact, wd.moments):
        a.setflags(write=False)
    return v, f, wd, pts, exact


def _meshes():
    out = {name: make() for name, make in D.MESHES.items()}
    out.update({f"small{F}": B.small(F) for F in (0, 1, 3, 4, 5, 8, 9, 17)})
    out.update(all_invalid=B.all_invalid(), doubled=B.doubled(), cube=D.cube(), open_cube=W.open_cube())
    return out


# ------------------------------------------------------------------------------------------------ the mirror
def test_known_values():
    v, f = D.cube()
    assert abs(W.exact_sum(CUBE_CENTRE, v, f)[0] - 1.0) < 1e-12                              # inside a closed mesh
    outside = np.array([[0.0, 0.75, 3.5], [9.0, -4.0, 1.0]], np.float32)
    assert np.abs(W.exact_sum(outside, v, f)).max() < 1e-12
    vo, fo = W.open_cube()
    assert len(fo) == 10 and abs(W.exact_sum(CUBE_CENTRE, vo, fo)[0] - 5.0 / 6.0) < 1e-12      # one of six sides is missing
    origin = np.zeros((1, 3), np.float32)
    assert abs(W.exact_sum(origin, *W.octant_triangle())[0] - 0.125) < 1e-12                 # an eighth of the sphere,
    assert abs(W.exact_sum(origin, *W.octant_triangle(flip=True))[0] + 0.125) < 1e-12        # signed by the order of its corners
    in_plane = np.array([[0.5, 0.5, 0.0], [2.0, -1.0, 0.0], [1.0, 0.0, 0.0]], np.float32)     # x + y + z = 1 exactly
    assert (W.exact_sum(in_plane, *W.octant_triangle()) == 0.0).all()
    # the scalar term the walk uses says the same
    a, b, c = ([float(x) for x in r] for r in W.octant_triangle()[0])
    assert abs(W.solid_angle([0.0] * 3, a, b, c) - 0.5 * np.pi) < 1e-12 and W.solid_angle([0.5, 0.5, 0.0], a, b, c) == 0.0
    assert np.isnan(W.exact_sum(np.array([[0.0, np.nan, 0.0]], np.float32), v, f)[0])


@pytest.mark.parametrize("name", sorted(_meshes()))
def test_the_walk_without_dipoles_equals_the_sum_in_face_order(name):
    v, f = _meshes()[name]
    pts = np.concatenate([D.query_points(v, f, 300, 5), B.far_points()])
    if name == "sphere24":
        pts = np.concatenate([pts[::10][:31], pts[7:8]])              # 32 points, the NaN one among them: every point visits every face
    wd = W.Winding(v, f)
    w, visits = wd.query(pts, np.inf)
    want = W.exact_sum(pts, v, f)
    fin = np.isfinite(pts).all(1)
    valid = int(D.corners(v, f)[0].sum())
    assert (~fin).sum() == 1 and np.isnan(w[~fin]).all() and np.isnan(want[~fin]).all() and not visits[~fin].any()
    assert wd.valid == valid and (visits[fin] == (valid, 0)).all()
    worst = np.abs(w[fin] - want[fin]).max()
    assert worst <= len(f) * 2.0 ** -50, (name, worst)
    if valid == 0:
        assert (w[fin] == 0.0).all() and (want[fin] == 0.0).all()


@pytest.mark.parametrize("name", sorted(_meshes()))
def test_root_moments(name):
    v, f = _meshes()[name]
    wd = W.Winding(v, f)
    ok, a, b, c, _ = D.corners(v, f)
    n, af, _ = W.face_terms(a[ok], b[ok], c[ok])
    root = wd.moments[1]
    area = float(af.sum())
    assert wd.moments.shape == (2 * wd.P, W.NODE_DOUBLES) and not wd.moments[0].any() and not wd.moments[:, 11].any()
    assert abs(root[W.A_AT] - area) <= 1e-12 * max(area, 1.0)
    assert np.abs(root[:3] - n.sum(0)).max() <= 1e-12 * max(area, 1.0)
    empty = wd.tree.nodes[:, 0] > wd.tree.nodes[:, 3]
    assert not wd.moments[empty].any() and (wd.moments[~empty, W.A_AT] > 0).all()
    if name in ("tetrahedron", "sphere12", "sphere24", "cube", "doubled"):                     # closed: the area vectors cancel
        assert np.linalg.norm(root[:3]) < 1e-12 * area
    # every face of a node lies within r of its centre
    for s, face in enumerate(wd.tree.order):
        if face < 0:
            continue
        i = wd.P + s // B.LEAF
        corner = np.stack([a[face], b[face], c[face]]).astype(np.float64)
        while i >= 1:
            m = wd.moments[i]
            assert np.sqrt(((corner - m[3:6]) ** 2).sum(1)).max() <= m[W.R_AT] * (1 + 1e-12), (name, face, i)
            i //= 2


def test_dipole_error_on_sphere24():
    _, _, wd, pts, exact = _sphere24()
    fin = np.isfinite(pts).all(1)
    err = {}
    for beta in (2.0, 3.0):
        w, _ = wd.query(pts, beta)
        err[beta] = np.abs(w[fin] - exact[fin]).max()
    print("sphere24: worst dipole error", err)
    assert err[2.0] < SPHERE24_DIPOLE_BAR and err[3.0] < err[2.0]
    assert abs(err[2.0] - SPHERE24_DIPOLE_ERR) < 1e-4                 # the figure DESIGN.md section 40 quotes


def test_a_query_evaluates_a_small_share_of_the_faces():
    """Agreement with the exact sum cannot see a walk that stopped approximating: it would only be more exact."""
    _, f, wd, pts, _ = _sphere24()
    fin = np.isfinite(pts).all(1)
    _, visits = wd.query(pts, 2.0)
    mean = visits[fin, 0].mean()
    print("sphere24: mean faces evaluated", mean, "of", len(f), "nodes approximated", visits[fin, 1].mean())
    assert wd.tree.nL == 1016 and mean <= SPHERE24_CAP < 0.13 * len(f)
    assert abs(mean - SPHERE24_MEAN_FACES) < 0.01                     # the figure DESIGN.md section 40 quotes
    assert (visits[fin, 1] >= 1).all() and not visits[~fin].any()


def test_remesh_of_the_open_cube_is_closed():
    vo, fo = W.open_cube()
    counts = M.undirected_edge_counts(fo)
    assert (counts == 1).sum() == 4 and (counts == 2).sum() == 13     # the hole's four boundary edges
    vol, w64 = W.Winding(vo, fo).volume(16, D.LO, D.HI, 2.0)
    gap = np.abs(w64 - 0.5).min()
    print("open cube, R = 16: the lattice value closest to 0.5 is", gap, "away")
    assert gap > 1e-6                                                 # no lattice value on the level itself (measured: 0.028)
    mv, mf, _ = M.marching_cubes(vol, 0.5, D.LO, D.HI)
    assert len(mf) > 0 and (M.undirected_edge_counts(mf) == 2).all() and M.closed_and_oriented(mf)
    # one piece with the topology of a sphere, oriented outward, and no vertex further than a cell from the unit cube: the level
    # lies between a lattice point inside (w > 0.5) and a neighbour outside
    h = (np.array(D.HI) - np.array(D.LO)).max() / 16
    assert M.euler(mv, mf) == 2 and M.enclosed_volume(mv, mf) > 0.0
    assert (np.abs(mv - vo.mean(0)).max(1) <= 0.5 + h).all()


# ------------------------------------------------------------------------------------------------ workspace carve
SIZES = [0, 1, 4, 5, 1 << 24]


@pytest.fixture(scope="module")
def carved(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("winding_ws") / "winding_ws_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "winding_ws_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    ws, bad, consts, cur = {}, None, None, None
    for ln in out.stdout.splitlines():
        w = ln.split()
        if w[0] == "ws":
            cur = ws[int(w[1])] = {k: int(x) for k, x in zip(w[2::2], w[3::2])}
        elif w[0] == "region":
            cur["region"] = (int(w[2]), int(w[3]))
        elif w[0] == "last_record_end":
            cur["last_record_end"] = int(w[1])
        elif w[0] == "bad":
            bad = [int(x) for x in w[1:]]
        elif w[0] == "consts":
            consts = [int(x) for x in w[1:]]
        else:
            raise AssertionError(ln)
    return ws, bad, consts


def test_workspace_carve(carved):
    ws, bad, consts = carved
    assert sorted(ws) == SIZES and bad == [-1, -1, -1]
    assert consts == [W.NODE_DOUBLES, W.N_AT, W.C_AT, W.R_AT, W.A_AT, W.S_AT]
    for F in SIZES:
        w = ws[F]
        _, P, depth, launches = B.tree_shape(F)
        assert (w["P"], w["depth"], w["launches"]) == (P, depth, launches) == (w["bvh_P"], w["bvh_depth"], w["bvh_launches"])
        assert w["bytes"] == w["total"] == 2 * P * 96 and w["bytes"] % 16 == 0
        assert w["region"] == (0, 2 * P * 96) and w["last_record_end"] == w["bytes"]
    assert ws[0]["bytes"] == 192 and ws[5]["bytes"] == 384 and ws[1 << 24]["bytes"] == 2 * (1 << 22) * 96


# ------------------------------------------------------------------------------------------------ host-side API
def test_arguments_are_checked():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = (torch.from_numpy(a.copy()) for a in S.sphere(12))
    good = E.Mesh(v, f, torch.zeros_like(v), None)
    pts = torch.zeros(5, 3)
    assert E.check_winding_args(good, S.LO, S.HI) == (2.0, S.LO, S.HI, 2)
    assert E.check_winding_args(good, S.LO, S.HI, float("inf"), 16, pts) == (float("inf"), S.LO, S.HI, 16)
    assert E.check_winding_args(good, S.LO, S.HI, 1) == (1.0, S.LO, S.HI, 2)
    for beta in (float("nan"), 0.999, 0, -2.0, float("-inf"), None, "2", True, [2.0]):
        with pytest.raises(ValueError, match="beta"):
            E.check_winding_args(good, S.LO, S.HI, beta)
        for call in (lambda: E.winding_number(pts, good, S.LO, S.HI, beta), lambda: E.winding_volume(good, 8, S.LO, S.HI, beta),
                     lambda: E.remesh(good, 8, S.LO, S.HI, beta), lambda: E.signed_distance(pts, good, S.LO, S.HI, beta)):
            with pytest.raises(ValueError, match="beta"):
                call()
    for R in (1, 513, 2.5, True, None):
        with pytest.raises(ValueError, match="resolution"):
            E.winding_volume(good, R, S.LO, S.HI)
        with pytest.raises(ValueError, match="resolution"):
            E.remesh(good, R, S.LO, S.HI)
    for lo, hi in (([0.0] * 3, [0.0] * 3), ([0.0] * 3, [1.0, 1.0, float("nan")]), ([0.0] * 2, [1.0] * 2), (S.HI, S.LO)):
        with pytest.raises(ValueError, match="box"):
            E.check_winding_args(good, lo, hi)
        with pytest.raises(ValueError, match="box"):
            E.MeshWinding(good, lo, hi)
    for m in (good._replace(verts=v.double()), good._replace(faces=f.long()), (v, f), None):
        with pytest.raises(ValueError):
            E.check_winding_args(m, S.LO, S.HI)
        with pytest.raises(ValueError):
            E.MeshWinding(m, S.LO, S.HI)
    for p in (pts.double(), pts[:, :2], pts.numpy(), pts.t().contiguous().t(), torch.zeros(5)):
        with pytest.raises(ValueError, match="points"):
            E.check_winding_args(good, S.LO, S.HI, points=p)
        with pytest.raises(ValueError, match="points"):
            E.signed_distance(p, good, S.LO, S.HI)
    for bad in ("BVH", "tree", "", None, 1):
        with pytest.raises(ValueError, match="index"):
            E.signed_distance(pts, good, S.LO, S.HI, index=bad)
    for kw in ({"min_component": -1}, {"largest_only": 1}, {"opening_radius": 17}):            # before anything is computed
        with pytest.raises(ValueError):
            E.remesh(good, 8, S.LO, S.HI, **kw)
    with pytest.raises(ValueError, match="bvh"):
        E.MeshWinding(good, S.LO, S.HI, bvh=object())
    assert E.WINDING_INSIDE == 0.5 and E.WINDING_NODE_DOUBLES == W.NODE_DOUBLES


def test_trainer_methods_and_mesh_tool_options():
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    sig = {name: [(p.name, p.default) for p in inspect.signature(getattr(Trainer, name)).parameters.values()][1:]
           for name in ("remesh", "signed_distance", "mesh_distance")}
    assert sig["remesh"] == [("mesh", inspect.Parameter.empty), ("resolution", 256), ("aabb", None), ("beta", 2.0),
                             ("min_component", 0), ("largest_only", False), ("opening_radius", 0)]
    assert sig["signed_distance"] == [("mesh", inspect.Parameter.empty), ("points", inspect.Parameter.empty), ("aabb", None),
                                      ("beta", 2.0)]
    assert [n for n, _ in sig["mesh_distance"]] == ["mesh", "other", "n", "tau", "seed", "aabb"]
    import importlib.util
    spec = importlib.util.spec_from_file_location("ngp_mesh_tool_winding", os.path.join(ROOT, "tools", "ngp_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.parser().parse_args([])
    assert args.winding is False and args.winding_beta == 2.0
    args = tool.parser().parse_args(["--winding", "--winding-beta", "3"])
    assert args.winding is True and args.winding_beta == 3.0


def test_c_entries_refuse_before_any_device_work():
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    p = C.c_void_p(4096)                                               # never dereferenced: every call below is refused
    odd = C.c_void_p(4096 + 8)
    big = (1 << 24) + 1

    def build(verts=p, V=4, faces=p, F=4, bvh=p, ws=p):
        return L.nerf_winding_build(verts, V, faces, F, bvh, ws, None)

    def query(pts=p, n=5, verts=p, V=4, faces=p, F=4, bvh=p, ws=p, beta=2.0, w=p, visits=p):
        return L.nerf_winding_query(pts, n, verts, V, faces, F, bvh, ws, beta, w, visits, None)

    sizes = [{"V": big}, {"V": -1}, {"F": big}, {"F": -1}]
    betas = [{"beta": float("nan")}, {"beta": 0.999}, {"beta": 0.0}, {"beta": -2.0}, {"beta": float("-inf")}]
    for fn, name, kws in ((build, b"nerf_winding_build", sizes + [{"ws": odd}, {"bvh": odd}]),
                          (query, b"nerf_winding_query", sizes + betas + [{"n": -1}, {"n": (1 << 30) + 1}, {"ws": odd}, {"bvh": odd}])):
        for kw in kws:
            assert fn(**kw) == E_SHAPE, (name, kw)
            assert name in L.nerf_last_error()
    for fn, kws in ((build, [{"verts": None}, {"faces": None}, {"bvh": None}, {"ws": None}]),
                    (query, [{"pts": None}, {"verts": None}, {"faces": None}, {"bvh": None}, {"ws": None}, {"w": None},
                             {"visits": None}, {"bvh": None, "F": 0}])):
        for kw in kws:
            assert fn(**kw) == E_NULL, (fn.__name__, kw)
    # a bad beta is refused even where nothing would be launched; nothing to do is no error, whatever the pointers
    assert query(n=0, beta=float("nan")) == E_SHAPE
    assert build(F=0, verts=None, faces=None, bvh=None, ws=None) == 0
    assert query(n=0, pts=None, w=None, visits=None, bvh=None, ws=None) == 0 and query(n=0, beta=float("inf")) == 0
    for bad in (-1, big):
        assert L.nerf_winding_workspace_bytes(bad) == -1
    assert L.nerf_winding_workspace_bytes(0) == 192 and L.nerf_winding_workspace_bytes(5) == 384
    assert L.nerf_winding_workspace_bytes(1 << 24) == 2 * (1 << 22) * 96


def test_header_section_bindings_and_makefile():
    from nerf_meets_mlx_amd import _native
    from nerf_meets_mlx_amd.engine import mesh as E
    text = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    start = text.index("/* ---------------------------------------------------------------- mesh winding number (no reference counterpart)")
    bvh = text.index("mesh BVH (no reference counterpart)")
    assert text.index("/* ----", bvh) == start < text.index("texture atlas (no reference counterpart)")     # directly behind
    section = text[start + 3:text.index("/* ----", start + 3)]
    decl = re.sub(r"/\*.*?\*/", "", "/*" + section, flags=re.S)
    assert sorted(set(re.findall(r"\b(nerf_[a-z_]+)\s*\(", decl))) == ENTRIES
    lib = _native.lib()
    for e in ENTRIES:
        assert e in _native.SIGNATURES and hasattr(lib, e)
    assert _native.SIGNATURES["nerf_winding_query"][1][8] is C.c_double
    assert lib.nerf_abi_version() == 3 and "#define NERF_ABI_VERSION 3" in text
    flat = section.replace("\n * ", " ").replace("\n *", " ")
    flat = re.sub(r"\s+", " ", flat)
    for word in ("2 atan2(det, den)", "det == 0", "w > 0.5", "convention", "4 pi = 12.566370614359172", "left + right",
                 "farthest corner", "strictly", "a NaN product never approximates", "stackless", "no trail word",
                 "while the node is odd, halve it", "(NaN 0x7FF8000000000000, 0, 0)", "NERF_ABI_VERSION stays 3", "Not done",
                 "no quadrupole or higher terms", "no narrow band", "no culling of faces that lie inside the solid",
                 "still no ray casting", "Barill", "Jacobson"):
        assert word in flat, word
    csrc = os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    hdrs = next(ln for ln in mk.splitlines() if ln.startswith("HDRS"))
    assert "winding.hip" in srcs.split() and "bvh.hip" in srcs.split()
    assert "winding_ws.h" in hdrs.split() and "bvh_ws.h" in hdrs.split() and "distance.h" in hdrs.split() and "bvh_tree.h" in hdrs.split()
    assert not re.search(r"FLAGS_winding", mk)                                            # the default flags, -ffp-contract=off among them
    src = open(os.path.join(csrc, "winding.hip")).read()
    kernels = sorted(set(re.findall(r"\b(\w+_kernel)\(", src)))
    assert kernels == ["wind_leaves_kernel", "wind_query_kernel"]
    assert not re.search(r"\batomic\w*\(", src) and "__shared__" not in src                # no atomics at all, no LDS
    # the level and top kernels are the hierarchy's, written once in bvh_tree.h and held to the same two assertions
    tree = open(os.path.join(csrc, "bvh_tree.h")).read()
    assert '#include "bvh_tree.h"' in src and "tree_reduce(" in src and "tree_level_kernel" not in src and "tree_top_kernel" not in src
    assert sorted(set(re.findall(r"\b(\w+_kernel)\(", tree))) == ["tree_level_kernel", "tree_top_kernel"]
    assert not re.search(r"\batomic\w*\(", tree) and "__shared__" not in tree
    assert '#include "distance.h"' in src and '#include "bvh_ws.h"' in open(os.path.join(csrc, "winding_ws.h")).read()
    assert "dist_face(" in src and "dist_load(" in src
    ws = open(os.path.join(csrc, "winding_ws.h")).read()
    assert "hip" not in re.sub(r"//.*", "", ws).lower()                                   # compiles without HIP
    module = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "engine", "mesh", "winding.py")).read()
    for name in ("MeshWinding", "winding_number", "winding_volume", "remesh", "signed_distance", "check_winding_args"):
        assert hasattr(E, name) and name in module
    assert "distance (sample_surface, MeshIndex, mesh_distance)" in E.__doc__ and "MeshBVH" in E.__doc__ and "MeshWinding" in E.__doc__
