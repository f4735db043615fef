"""The mesh BVH without a GPU: the numpy mirror (tests/_bvh_ref.py) of include/nerf_hip.h "mesh BVH" held to the brute force of
tests/_distance_ref.py bit for bit, the tree's invariants, a cap on the leaves a query enters, the closest point, the workspace
carve of csrc/bvh_ws.h in a stand-alone program built with the host compiler and -fsanitize=address,undefined
(tests/bvh_ws_check.cpp), the argument checks of engine.mesh and of the C entries (all of them return before any device work), and
the header / binding / Makefile bookkeeping.  The GPU side is held to the mirror bit for bit in tests/test_gpu_bvh.py."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import _bvh_ref as B
from tests import _distance_ref as D
from tests import _smooth_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE = -1, -2
ENTRIES = ["nerf_bvh_build", "nerf_bvh_keys", "nerf_bvh_query", "nerf_bvh_workspace_bytes", "nerf_closest_points"]
# The mirror's own count on sphere24 (F = 4064, nL = 1016 leaves) with D.query_points(.., 300, 5): 14.02 leaves entered per finite
# point (56.08 faces tested).  The cap is twice that: a walk that stopped pruning would enter every non-empty leaf, 1016.
SPHERE24_MEAN_LEAVES, SPHERE24_CAP = 14.02, 28.04


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(verts, faces, the mirror's tree, points, brute force, the walk's answers): computed once, shared, read-only."""
    v, f = D.MESHES[name]()
    pts = np.concatenate([D.query_points(v, f, 300, 5), B.far_points()])
    want = D.brute_force(pts, v, f)
    tree = B.Tree(v, f)
    got = tree.query(pts)
    for a in (pts,) + want + got:
        a.setflags(write=False)
    return v, f, tree, pts, want, got


# ------------------------------------------------------------------------------------------------ the mirror
@pytest.mark.parametrize("name", sorted(D.MESHES))
def test_the_emulated_traversal_equals_the_brute_force_bit_for_bit(name):
    v, f, tree, pts, (d2, fc), (gd, gf, leaves, cands) = _case(name)
    assert len(pts) == 307 and np.isnan(pts).any(1).sum() == 1
    ext = np.array(D.HI) - np.array(D.LO)
    far = pts[300:]
    assert (np.maximum(np.array(D.LO) - far, far - np.array(D.HI)).max(1) >= 99.0 * ext.min()).all()      # 100 box widths away
    bad = (_bits(gd) != _bits(d2)) | (gf != fc)
    assert not bad.any(), (name, np.nonzero(bad)[0][:6], gd[bad][:6], d2[bad][:6], gf[bad][:6], fc[bad][:6])
    fin = np.isfinite(pts).all(1)
    assert (leaves[fin] >= 1).all() and (cands <= B.LEAF * leaves).all() and not leaves[~fin].any()
    print(name, "F", len(f), "leaves", tree.nL, "mean leaves entered", leaves[fin].mean(), "faces tested", cands[fin].mean(),
          "far points", leaves[300:].mean())


def test_a_query_enters_a_small_share_of_the_leaves():
    """Bit equality cannot see a walk that stopped pruning: it would still find the minimum.  The cap is twice the mirror's own
    mean on this mesh and these points (see SPHERE24_MEAN_LEAVES), 2.8 % of the 1016 leaves."""
    _, _, tree, pts, _, (_, _, leaves, cands) = _case("sphere24")
    fin = np.isfinite(pts[:300]).all(1)
    mean = leaves[:300][fin].mean()
    print("sphere24: mean leaves entered", mean, "of", tree.nL, "faces tested", cands[:300][fin].mean())
    assert tree.nL == 1016 and mean <= SPHERE24_CAP < 0.03 * tree.nL
    assert abs(mean - SPHERE24_MEAN_LEAVES) < 0.01                   # the figure DESIGN.md section 38 quotes
    assert leaves[300:].max() <= SPHERE24_CAP                        # 100 box widths away costs no more


@pytest.mark.parametrize("name", sorted(D.MESHES))
def test_keys_are_unique_and_every_face_lies_in_its_ancestors(name):
    v, f, tree, _, _, _ = _case(name)
    ok, a, b, c, _ = D.corners(v, f)
    k = B.keys(v, f, D.LO, D.HI)
    assert k.dtype == np.int64 and len(np.unique(k)) == len(k) and (k >= 0).all()
    assert np.array_equal(k & ((1 << 24) - 1), np.arange(len(f))) and np.array_equal((k >> 24) == B.INVALID_CODE, ~ok)
    assert ((k >> 24)[ok] < B.INVALID_CODE).all()
    o = tree.order
    assert sorted(o[o >= 0]) == list(np.nonzero(ok)[0]) and (o[int(ok.sum()):] == -1).all() and (o[:int(ok.sum())] >= 0).all()
    nL, P, depth, launches = B.tree_shape(len(f))
    assert tree.nodes.shape == (2 * P, 6) and P >= max(nL, 1) and P < 2 * max(nL, 1) and launches <= 23 and depth <= 22
    assert np.isposinf(tree.nodes[0, :3]).all() and np.isneginf(tree.nodes[0, 3:]).all()
    for s, face in enumerate(o):
        if face < 0:
            continue
        corner = np.stack([a[face], b[face], c[face]])
        i = P + s // B.LEAF
        while i >= 1:
            assert (tree.nodes[i, :3] <= corner.min(0)).all() and (corner.max(0) <= tree.nodes[i, 3:]).all(), (name, face, i)
            i //= 2
    # the boxes are tight: the root is the exact bounding box of the valid faces
    if ok.any():
        every = np.concatenate([a[ok], b[ok], c[ok]])
        assert np.array_equal(_bits(tree.nodes[1]), _bits(np.concatenate([every.min(0), every.max(0)])))


def test_morton_codes_interleave_x_lowest():
    assert [int(B.morton([x, y, z])) for x, y, z in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (4095, 4095, 4095), (4095, 0, 0))] \
        == [1, 2, 4, 8, (1 << 36) - 1, 0x249249249]
    lo, hi = D.LO, D.HI
    c = B.cells_of(np.array([lo, hi, [(l + h) / 2 for l, h in zip(lo, hi)], [l - 5 for l in lo], [h + 5 for h in hi]]), lo, hi)
    assert c.tolist() == [[0] * 3, [4095] * 3, [2048] * 3, [0] * 3, [4095] * 3]
    assert [B.tree_shape(F) for F in (0, 1, 3, 4, 5, 8, 9, 17, 4064, 8128, 1 << 24)] == \
        [(0, 1, 0, 2), (1, 1, 0, 2), (1, 1, 0, 2), (1, 1, 0, 2), (2, 2, 1, 2), (2, 2, 1, 2), (3, 4, 2, 2), (5, 8, 3, 2),
         (1016, 1024, 10, 3), (2032, 2048, 11, 4), (1 << 22, 1 << 22, 22, 15)]


@pytest.mark.parametrize("name", sorted(D.MESHES))
def test_closest_recomputes_dist2_bit_for_bit(name):
    v, f, _, pts, (d2, fc), _ = _case(name)
    q = B.closest(pts, v, f, fc)
    hit = fc >= 0
    assert hit.sum() >= 300 and np.array_equal(_bits(B.dist2_of(pts, q)[hit]), _bits(d2[hit]))
    assert np.isnan(q[~hit]).all() and np.isfinite(q[hit]).all()
    ok = D.corners(v, f)[0]
    odd = np.array([-1, len(f), -7, 1 << 30] + list(np.nonzero(~ok)[0][:3]), np.int64)
    assert np.isnan(B.closest(pts[:len(odd)], v, f, odd)).all()
    on = B.closest(v[f[ok][:20, 0]], v, f, np.nonzero(ok)[0][:20])     # a corner is its own closest point
    assert np.array_equal(_bits(on), _bits(v[f[ok][:20, 0]]))


# ------------------------------------------------------------------------------------------------ workspace carve
SIZES = [0, 1, 4, 5, 1 << 24]


@pytest.fixture(scope="module")
def carved(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("bvh_ws") / "bvh_ws_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "bvh_ws_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    ws, bad, consts, cur = {}, None, None, None
    for ln in out.stdout.splitlines():
        w = ln.split()
        if w[0] == "ws":
            cur = ws[int(w[1])] = {k: int(x) for k, x in zip(w[2::2], w[3::2])}
            cur["regions"] = {}
        elif w[0] == "region":
            cur["regions"][w[1]] = (int(w[2]), int(w[3]))
        elif w[0] == "tiled":
            cur["tiled"], cur["last_leaf"] = int(w[1]), int(w[3])
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
    assert consts == [B.LEAF, 6, 9, B.CELLS, B.INVALID_CODE, B.KEY_SHIFT]
    for F in SIZES:
        w = ws[F]
        nL, P, depth, launches = B.tree_shape(F)
        assert (w["leaves"], w["P"], w["depth"], w["launches"]) == (nL, P, depth, launches) and launches <= 23
        assert w["bytes"] == w["total"] and w["tiled"] == 1 and w["last_leaf"] == (P + (F - 1) // 4 if F else -1) < 2 * P
        end = 0
        for name in ("nodes", "order"):                              # in order, 16-byte aligned, no overlap, nothing past the end
            at, size = w["regions"][name]
            assert at % 16 == 0 and at >= end and at - end < 16
            end = at + size
        assert end <= w["bytes"] < end + 16
        assert w["regions"]["nodes"][1] == 2 * P * 24 and w["regions"]["order"][1] == 4 * F
    assert ws[1 << 24]["bytes"] == 2 * (1 << 22) * 24 + 4 * (1 << 24) and ws[0]["bytes"] == 48


# ------------------------------------------------------------------------------------------------ host-side API
def test_index_argument_is_checked():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = (torch.from_numpy(a.copy()) for a in S.sphere(12))
    good = E.Mesh(v, f, torch.zeros_like(v), None)
    pts = torch.zeros(5, 3)
    assert E.DISTANCE_INDEXES == ("grid", "bvh") and [E.check_distance_index(i) for i in E.DISTANCE_INDEXES] == ["grid", "bvh"]
    for bad in ("BVH", "tree", "", None, 1, True, b"bvh"):
        with pytest.raises(ValueError, match="index"):
            E.check_distance_index(bad)
        with pytest.raises(ValueError, match="index"):
            E.point_mesh_distance(pts, good, S.LO, S.HI, index=bad)
        with pytest.raises(ValueError, match="index"):
            E.mesh_distance(good, good, 8, S.LO, S.HI, index=bad)
    with pytest.raises(ValueError, match="grid"):
        E.point_mesh_distance(pts, good, S.LO, S.HI, grid=4, index="bvh")       # a grid means nothing to the hierarchy
    # the one check of the arguments keeps its signature and its answer
    assert E.check_distance_args(good, 5, S.LO, S.HI) == (5, S.LO, S.HI, None, 0, None)
    for m in (good._replace(verts=v.double()), (v, f), None):
        with pytest.raises(ValueError):
            E.MeshBVH(m, S.LO, S.HI)
        with pytest.raises(ValueError):
            E.closest_points(m, pts, torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError):
        E.MeshBVH(good, [0.0] * 3, [0.0] * 3)
    for p, fc in ((pts.double(), torch.zeros(5, dtype=torch.int32)), (pts, torch.zeros(5, dtype=torch.int64)),
                  (pts, torch.zeros(4, dtype=torch.int32)), (pts[:, :2], torch.zeros(5, dtype=torch.int32)), (pts.numpy(), None)):
        with pytest.raises(ValueError):
            E.closest_points(good, p, fc)
    assert E.closest_points(good, pts[:0], torch.zeros(0, dtype=torch.int32)).shape == (0, 3)


def test_mesh_tool_has_the_index_option():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ngp_mesh_tool_bvh", os.path.join(ROOT, "tools", "ngp_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.parser().parse_args(["--distance"]).distance_index == "grid"
    assert tool.parser().parse_args(["--distance", "--distance-index", "bvh"]).distance_index == "bvh"
    with pytest.raises(SystemExit):
        tool.parser().parse_args(["--distance-index", "tree"])


def test_c_entries_refuse_before_any_device_work():
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    lo, hi = (C.c_float * 3)(*S.LO), (C.c_float * 3)(*S.HI)
    flat, nanbox = (C.c_float * 3)(1.5, -0.7, 3.1), (C.c_float * 3)(float("nan"), 2.3, 3.1)
    p = C.c_void_p(4096)                                               # never dereferenced: every call below is refused
    big = (1 << 24) + 1

    def keys(verts=p, V=4, faces=p, F=4, lo=lo, hi=hi, out=p):
        return L.nerf_bvh_keys(verts, V, faces, F, lo, hi, out, None)

    def build(verts=p, V=4, faces=p, F=4, keys=p, ws=p):
        return L.nerf_bvh_build(verts, V, faces, F, keys, ws, None)

    def query(pts=p, n=5, verts=p, V=4, faces=p, F=4, lo=lo, hi=hi, ws=p, d=p, face=p):
        return L.nerf_bvh_query(pts, n, verts, V, faces, F, lo, hi, ws, d, face, None)

    def closest(pts=p, n=5, verts=p, V=4, faces=p, F=4, face=p, out=p):
        return L.nerf_closest_points(pts, n, verts, V, faces, F, face, out, None)

    sizes = [{"V": big}, {"V": -1}, {"F": big}, {"F": -1}]
    box = [{"hi": flat}, {"hi": lo}, {"lo": nanbox}]
    odd = C.c_void_p(4096 + 8)
    for fn, name, kws in ((keys, b"nerf_bvh_keys", sizes + box), (build, b"nerf_bvh_build", sizes + [{"ws": odd}]),
                          (query, b"nerf_bvh_query", sizes + box + [{"n": -1}, {"n": (1 << 30) + 1}, {"ws": odd}]),
                          (closest, b"nerf_closest_points", sizes + [{"n": -1}, {"n": (1 << 30) + 1}])):
        for kw in kws:
            assert fn(**kw) == E_SHAPE, (name, kw)
            assert name in L.nerf_last_error()
    for fn, kws in ((keys, [{"verts": None}, {"faces": None}, {"out": None}, {"lo": None}, {"hi": None}]),
                    (build, [{"verts": None}, {"faces": None}, {"keys": None}, {"ws": None}, {"ws": None, "F": 0}]),
                    (query, [{"pts": None}, {"verts": None}, {"faces": None}, {"ws": None}, {"d": None}, {"face": None}, {"lo": None}]),
                    (closest, [{"pts": None}, {"verts": None}, {"faces": None}, {"face": None}, {"out": None}])):
        for kw in kws:
            assert fn(**kw) == E_NULL, (fn.__name__, kw)
    # nothing to do is no error, whatever the pointers
    assert keys(F=0, faces=None, out=None) == 0 and query(n=0, pts=None, d=None, face=None, ws=None) == 0
    assert closest(n=0, pts=None, face=None, out=None) == 0
    for bad in (-1, big):
        assert L.nerf_bvh_workspace_bytes(bad) == -1
    assert L.nerf_bvh_workspace_bytes(0) == 48 and L.nerf_bvh_workspace_bytes(5) == 2 * 2 * 24 + 32
    assert L.nerf_bvh_workspace_bytes(1 << 24) == 2 * (1 << 22) * 24 + 4 * (1 << 24)


def test_header_section_bindings_and_makefile():
    from nerf_meets_mlx_amd import _native
    from nerf_meets_mlx_amd.engine import mesh as E
    text = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    start = text.index("mesh BVH (no reference counterpart)")
    assert text.index("mesh distance (no reference counterpart)") < start < text.index("texture atlas (no reference counterpart)")
    section = text[start:text.index("/* ----", start)]
    decl = re.sub(r"/\*.*?\*/", "", "/*" + section, flags=re.S)
    assert sorted(set(re.findall(r"\b(nerf_[a-z_]+)\s*\(", decl))) == ENTRIES
    lib = _native.lib()
    for e in ENTRIES:
        assert e in _native.SIGNATURES and hasattr(lib, e)
    assert lib.nerf_abi_version() == 3 and "#define NERF_ABI_VERSION 3" in text
    for word in ("code 2^24 + f", "2^36", "LEAF = 4", "heap order", "(node >> k) ^ 1", "slack = 2^-18 S", "(m - slack)^2 (1 - 2^-20)",
                 "strictly", "stackless", "Not done", "Karras", "no signed distance", "no ray casting", "NERF_ABI_VERSION\n * stays 3"):
        assert word in section or word.replace("\n * ", " ") in section.replace("\n * ", " "), word
    csrc = os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    hdrs = next(ln for ln in mk.splitlines() if ln.startswith("HDRS"))
    assert "bvh.hip" in srcs.split() and "distance.hip" in srcs.split()
    assert "distance.h" in hdrs.split() and "bvh_ws.h" in hdrs.split() and "bvh_tree.h" in hdrs.split()
    assert not re.search(r"FLAGS_bvh", mk)                                               # the default flags, -ffp-contract=off among them
    src = open(os.path.join(csrc, "bvh.hip")).read()
    kernels = sorted(set(re.findall(r"\b(\w+_kernel)\(", src)))
    assert kernels == ["bvh_closest_kernel", "bvh_keys_kernel", "bvh_leaves_kernel", "bvh_query_kernel"]
    assert not re.search(r"\batomic\w*\(", src) and "__shared__" not in src                # no atomics at all, no LDS
    # the bottom-up pass is written once, in bvh_tree.h (a barrier between the top levels, no LDS), for both units on the tree
    tree = open(os.path.join(csrc, "bvh_tree.h")).read()
    wind = open(os.path.join(csrc, "winding.hip")).read()
    assert sorted(set(re.findall(r"\b(\w+_kernel)\(", tree))) == ["tree_level_kernel", "tree_top_kernel"]
    for name in ("tree_level_kernel", "tree_top_kernel"):
        assert len(re.findall(r"\b" + name + r"\(", tree)) == 1 and name not in src and name not in wind, name
    assert not re.search(r"\batomic\w*\(", tree) and "__shared__" not in tree and tree.count("__syncthreads()") == 1
    assert '#include "bvh_tree.h"' in src and '#include "bvh_tree.h"' in wind
    # the shared device code lives in one place, and distance.hip still has its own six kernels (its two offset kernels are scan.h's)
    shared = open(os.path.join(csrc, "distance.h")).read()
    dist = open(os.path.join(csrc, "distance.hip")).read()
    for name in ("dist_face", "dist_load", "point_triangle_closest", "point_triangle_d2", "dist_fold", "DIST_NONE", "dist_point",
                 "dist_stop", "box_abs", "points_check"):
        define = re.compile(r"(?:inline(?:__)?|constexpr)\s+\w+\s+" + name + r"\b")
        assert len(define.findall(shared)) == 1 and not define.search(dist) and not define.search(src) and not define.search(wind), name
    assert '#include "distance.h"' in dist and '#include "distance.h"' in src
    dk = sorted(set(re.findall(r"\b(\w+_kernel)\(", dist)))
    assert len(dk) == 6 and all(k.startswith("dist_") for k in dk) and dist.count("scan_offsets_") == 2
    for name in ("MeshBVH", "closest_points", "check_distance_index", "DISTANCE_INDEXES"):
        assert hasattr(E, name) and name in open(os.path.join(ROOT, "nerf_meets_mlx_amd", "engine", "mesh", "distance.py")).read()
    assert "distance (sample_surface, MeshIndex, mesh_distance)" in E.__doc__ and "MeshBVH" in E.__doc__
