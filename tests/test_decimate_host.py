"""Edge-collapse decimation without a GPU: the properties of the rule of include/nerf_hip.h "edge-collapse decimation" on its
numpy mirror (tests/_decimate_ref.py) -- the face count, the topology, the orientation, the boundary, the stops, the independence
of a round's collapses, and that the shared meshes reach every branch the GPU test then compares bit for bit -- and the host side of
the engine: argument checks, header section and bindings."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _decimate_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _targets(name):
    F = len(D.mesh(name)[1])
    return (F // 2, F // 10, 100, 4)


def _neighbours(faces, V):
    nb = [set() for _ in range(V)]
    for a, b, c in faces:
        nb[a] |= {b, c}
        nb[b] |= {a, c}
        nb[c] |= {a, b}
    return nb


@pytest.mark.parametrize("which", (0, 1, 2, 3))
@pytest.mark.parametrize("name", ["sphere", "box"])
def test_closed_meshes_reach_the_target_and_stay_closed_manifold_and_oriented(name, which):
    v, f, n, c = D.mesh(name)
    target = _targets(name)[which]
    (vo, fo, no, co), stats, _ = D.expected(name, target)
    assert len(fo) in (target, target - 1) and stats["stopped"] == "target" and stats["frozen"] == 0
    assert len(fo) == len(f) - 2 * sum(stats["collapses"])
    assert D.euler(fo) == 2 and D.all_edges_paired(fo)
    assert len(np.unique(fo)) == len(vo) and co.shape == vo.shape and np.isfinite(co).all()
    if name == "sphere":
        p = vo.astype(np.float64)
        fn = np.cross(p[fo[:, 1]] - p[fo[:, 0]], p[fo[:, 2]] - p[fo[:, 0]])
        out = p[fo].mean(1) - np.array([0.1, -0.05, 0.05])
        assert ((fn * out).sum(1) > 0.0).all()
        assert (np.abs(np.linalg.norm(p - [0.1, -0.05, 0.05], axis=1) - 0.6) < (0.05 if target >= 100 else 0.7)).all()


def test_a_boundary_stays_where_it_is():
    v, f, n, c = D.mesh("half")
    rim = D.boundary_vertices(f)
    assert len(rim) > 50
    for target in (300, 4):
        (vo, fo, no, co), stats, _ = D.expected("half", target)
        assert stats["frozen"] == len(rim)
        got = {tuple(x) for x in vo.view(np.int32).tolist()}
        assert all(tuple(x) in got for x in v[rim].view(np.int32).tolist())
        assert len(D.boundary_vertices(fo)) == len(rim)
    # the target below what the free vertices allow: every vertex left is on the rim or cannot go
    assert stats["stopped"] == "selected nothing" and stats["collapses"][-1] == 0 and len(fo) > 4


def test_a_mesh_of_frozen_vertices_comes_back_and_a_target_of_f_is_the_identity():
    k = 20
    sv = np.array([[0.04 * i - 0.4, 0.1 * j, 0.0] for i in range(k) for j in range(2)], np.float32)
    sf = np.array([t for i in range(k - 1) for t in ((2 * i, 2 * i + 2, 2 * i + 1), (2 * i + 1, 2 * i + 2, 2 * i + 3))], np.int32)
    (vo, fo, no, co), stats = D.decimate(sv, sf, np.zeros_like(sv), None, 4)
    assert stats == {"rounds": 1, "collapses": [0], "candidates": [0], "frozen": 2 * k, "stopped": "selected nothing"}
    assert np.array_equal(vo.view(np.int32), sv.view(np.int32)) and np.array_equal(fo, sf) and co is None
    v, f, n, c = D.mesh("box")
    for t in (len(f), len(f) + 5):
        (vo, fo, no, co), stats = D.decimate(v, f, n, c, t)
        same = [np.array_equal(np.asarray(x).view(np.int32), np.asarray(y).view(np.int32)) for x, y in ((vo, v), (fo, f), (no, n), (co, c))]
        assert all(same)
        assert stats["rounds"] == 0 and stats["stopped"] == "target"
    _, stats = D.decimate(v, f, n, c, 100, max_rounds=3)
    assert stats["rounds"] == 3 and stats["stopped"] == "max_rounds"


@pytest.mark.parametrize("name,target,passes", [("sphere", 4, 4), ("box", 100, 1), ("plate", 175, 4), ("noise", 925, 4),
                                                ("half", 4, 4), ("junk", 4, 4)])
def test_no_two_collapses_of_a_round_share_or_adjoin_a_vertex(name, target, passes):
    v = D.mesh(name)[0]
    _, stats, trace = D.expected(name, target, "quadric", True, passes)
    assert len(trace) == stats["rounds"] > 3
    for a, b, faces, c in trace:
        ends = np.r_[a, b]
        assert len(np.unique(ends)) == len(ends)
        nb = _neighbours(faces.tolist(), len(v))
        owner = {}
        for i, (x, y) in enumerate(zip(a.tolist(), b.tolist())):
            assert c["cand"][np.flatnonzero((c["a"] == x) & (c["b"] == y))[0]]
            for w in {x, y} | nb[x] | nb[y]:                # its ends and their rings: nobody else's end
                owner.setdefault(w, set()).add(i)
        for e in ends.tolist():
            assert len(owner[e]) == 1


def test_the_shared_meshes_reach_every_branch():
    """What tests/test_gpu_decimate.py compares bit for bit: a trim round, passes that find blocked vertices, frozen vertices, the
    midpoint fallback, rejected flips, rejected links, dropped faces."""
    seen = {"links": 0, "flips": 0, "fallbacks": 0, "trimmed": 0}
    for name in ("sphere", "box", "plate", "noise"):
        for target in _targets(name)[:3]:
            _, stats, trace = D.expected(name, target)
            for _, _, _, c in trace:
                for k in ("links", "flips", "fallbacks"):
                    seen[k] += c["branches"][k]
                seen["trimmed"] += c["trimmed"]
    assert all(n > 0 for n in seen.values()), seen
    one = D.expected("sphere", 346, "quadric", True, 1)[1]
    four = D.expected("sphere", 346, "quadric", True, 4)[1]
    assert one["rounds"] > four["rounds"] and one["collapses"][0] < four["collapses"][0]     # passes 2.. pick beside blocked rings
    assert D.expected("noise", 925)[1]["frozen"] > 0
    v, f, n, c = D.mesh("junk")
    (vo, fo, no, co), stats, _ = D.expected("junk", 500)
    assert stats["frozen"] > 0 and len(fo) in (499, 500)
    bad = ~np.isfinite(v).all(1)
    kept = {tuple(x) for x in vo.view(np.int32).tolist()}
    used = np.unique(D._valid_faces(f, len(v)))
    assert all(tuple(x) in kept for x in v[bad & np.isin(np.arange(len(v)), used)].view(np.int32).tolist())


def test_midpoint_placement_and_colours():
    (vq, fq, _, cq), sq, _ = D.expected("box", 196, "quadric", True, 4)
    (vm, fm, _, cm), sm, _ = D.expected("box", 196, "midpoint", True, 4)
    assert len(fm) in (195, 196) and not np.array_equal(vq, vm)
    # the quadric keeps the box's corners and faces, the midpoint rounds them
    eq, em = D.S.box_errors(vq), D.S.box_errors(vm)
    print("box errors (corner, surface): quadric", eq, "midpoint", em)
    assert eq[0] < em[0] and eq[1] < em[1]
    (_, f2, _, c2), _, _ = D.expected("box", 196, "quadric", False, 4)
    assert c2 is None and np.array_equal(f2, fq)
    col = D.mesh("box")[3]
    assert float(col.min()) - 1e-6 <= float(cq.min()) and float(cq.max()) <= float(col.max()) + 1e-6


def test_argument_checks():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f, n, c = (torch.from_numpy(np.array(a)) for a in D.mesh("box"))
    m = E.Mesh(v, f, n, c)
    assert E.check_decimate_args(m, 100, D.LO, D.HI) == (100, D.LO, D.HI, 1, 4, 1024)
    assert E.check_decimate_args(m, 4, D.LO, D.HI, "midpoint", 16, 1)[3:] == (0, 16, 1)
    for bad in ({"mesh": (v, f)}, {"target_faces": 3}, {"target_faces": 0}, {"target_faces": 100.0}, {"target_faces": True},
                {"passes": 0}, {"passes": 17}, {"passes": 2.5}, {"max_rounds": 0}, {"lo": [1.0, -1.0, -1.0]}, {"lo": [-1.0, -1.0]},
                {"hi": [float("inf"), 1.0, 1.0]}, {"placement": "mean"}, {"placement": None},
                {"mesh": E.Mesh(v, f.long(), n, c)}, {"mesh": E.Mesh(v.double(), f, n, c)}, {"mesh": E.Mesh(v, f, n[:-1], c)}):
        kw = {"mesh": m, "target_faces": 100, "lo": D.LO, "hi": D.HI, **bad}
        with pytest.raises(ValueError):
            E.check_decimate_args(**kw)
        with pytest.raises(ValueError):                      # before any device work: these tensors live on the host
            E.decimate(**kw)
    same, stats = E.decimate(m, len(f), D.LO, D.HI)          # the identity needs no device either
    assert same is m and stats == E.DecimateStats(0, [], [], 0, "target")
    assert E.DECIMATE_PLACEMENTS == D.PLACEMENTS and E.DECIMATE_STOPS == D.STOPS


@pytest.mark.parametrize("V,F", [(1, 1), (3, 1), (255, 257), (1 << 24, 1 << 24)])
def test_workspace_bytes_region_by_region(V, F):
    """nerf_decimate_workspace_bytes in closed form: the regions of the workspace in their order, each rounded up to 8 bytes;
    H = 3 F half-edges, nb(n) workgroups of 256 items."""
    from nerf_meets_mlx_amd import _native as N
    r8 = lambda b: (b + 7) & ~7
    nb = lambda n: (n + 255) // 256
    H = 3 * F
    want = (r8(8 * 8) + r8(8 * nb(V)) + r8(8 * nb(F)) + r8(8 * nb(H))            # cnt, blk_v, blk_f, blk_h
            + r8(8 * 10 * V) + r8(8 * 3 * V) + 2 * r8(8 * V) + r8(8 * H)         # Q, col, m1, m2, ekey
            + r8(12 * V) + 2 * r8(12 * F)                                        # pos, the two face lists
            + 2 * r8(4 * V) + r8(4 * 2 * V) + 5 * r8(4 * V)                      # mcnt, remap, vstart + vend, frozen ... newid
            + 4 * r8(4 * H))                                                     # ea, eb, sel, inc
    assert N.lib().nerf_decimate_workspace_bytes(V, F) == want


def test_header_section_and_bindings():
    from nerf_meets_mlx_amd import _native as N
    h = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    sec = h[h.index("edge-collapse decimation (no reference counterpart)"):h.index("mesh distance (no reference counterpart)")]
    for word in ("Independence", "link condition", "0x9E3779B1", "Not done", "tests/_decimate_ref.py", "DOES\n *             depend"):
        assert word in sec, word
    names = sorted(set(re.findall(r"\b(nerf_decimate_\w+)\(", sec)))
    assert len(names) == 9
    for name in names:
        assert name in N.SIGNATURES
    src = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "decimate.hip")).read()
    assert all(f'extern "C" int{"64_t" if n.endswith("bytes") else ""} {n}(' in src for n in names)
    assert "atomicAdd" not in src and "decimate.hip" in open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "Makefile")).read()
    assert int(re.search(r"#define NERF_DECIMATE_QUADRIC (\d)", h).group(1)) == D.PLACEMENTS["quadric"]
    assert int(re.search(r"#define NERF_DECIMATE_MIDPOINT (\d)", h).group(1)) == D.PLACEMENTS["midpoint"]
