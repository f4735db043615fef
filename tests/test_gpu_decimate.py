"""Edge-collapse decimation on the GPU (csrc/decimate.hip, engine/mesh/decimate.py, Trainer.decimate_mesh) against the numpy
reference of tests/_decimate_ref.py: vertex, normal and colour bits compared as integers, faces and the statistics exactly -- no
tolerance anywhere, the rule is exact -- into sentinel-filled outputs with one spare row and a poisoned workspace.  The meshes are
those of tests/test_decimate_host.py, which asserts that every branch fires on them: the trim round, blocked passes, frozen
vertices, the midpoint fallback, rejected flips and rejected links."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _decimate_ref as D
from tests._poison import NAN_BYTES, PATTERNS, bits_equal, poison_, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT32 = 0x7FE5A5A5
E_NULL, E_SHAPE = -1, -2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, order="C")).to(device=DEV, dtype=dtype).contiguous()


def _mesh(v, f, n, c):
    from nerf_meets_mlx_amd.engine import mesh as E
    return E.Mesh(_dev(v, torch.float32).reshape(-1, 3), _dev(f, torch.int32).reshape(-1, 3), _dev(n, torch.float32).reshape(-1, 3),
                  None if c is None else _dev(c, torch.float32).reshape(-1, 3))


def _decimate_poisoned(v, f, c, target, placement, passes, pattern=NAN_BYTES, lo=D.LO, hi=D.HI, max_rounds=1024):
    """The C calls of engine.mesh.decimate on numpy inputs, with a poisoned workspace, poisoned key buffers and sentinel outputs
    that carry one spare row each; ((verts, faces, normals, colors or None) as numpy arrays, stats as the reference's dict)."""
    from nerf_meets_mlx_amd import _native as N
    L, st = N.lib(), N.stream()
    tv, tf = _dev(v, torch.float32).reshape(-1, 3), _dev(f, torch.int32).reshape(-1, 3)
    tc = None if c is None else _dev(c, torch.float32).reshape(-1, 3)
    V, F = tv.shape[0], tf.shape[0]
    code, colors = D.PLACEMENTS[placement], int(c is not None)
    clo, chi = (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)
    nbytes = L.nerf_decimate_workspace_bytes(V, F)
    assert nbytes > 0
    ws = poison_(torch.empty(nbytes, dtype=torch.uint8, device=DEV), pattern)
    tot = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    N.check(L.nerf_decimate_begin(N.ptr(tv), N.ptr(tc), V, N.ptr(tf), F, N.ptr(ws), N.ptr(tot), st))
    cap, cur = int(tot[0]), 0
    stats = {"rounds": 0, "collapses": [], "candidates": [], "frozen": 0, "stopped": "target"}
    while cap > target:
        if stats["rounds"] == max_rounds:
            stats["stopped"] = "max_rounds"
            break
        keys = poison_(torch.empty(2, 3 * cap + 1, dtype=torch.int64, device=DEV), pattern)[:, :3 * cap].contiguous()
        sel = poison_(torch.empty(3 * cap + 1, dtype=torch.int64, device=DEV), pattern)
        N.check(L.nerf_decimate_keys(V, F, cap, cur, N.ptr(ws), N.ptr(keys), st))
        sk = torch.sort(keys, dim=1).values
        N.check(L.nerf_decimate_edges(V, F, cap, N.ptr(sk), N.ptr(ws), st))
        if stats["rounds"] == 0:
            N.check(L.nerf_decimate_quadrics(V, F, cur, clo, chi, N.ptr(ws), st))
        N.check(L.nerf_decimate_select(V, F, cap, cur, clo, chi, code, passes, N.ptr(ws), N.ptr(sel), st))
        assert bool((sel[3 * cap:].view(torch.uint8) == pattern).all())
        ss = torch.sort(sel[:3 * cap]).values
        N.check(L.nerf_decimate_apply(V, F, cap, cur, clo, chi, code, colors, target, N.ptr(ss), N.ptr(ws), N.ptr(tot), st))
        cap, n_sel, n_cand, n_frozen = tot.tolist()
        cur = 1 - cur
        if stats["rounds"] == 0:
            stats["frozen"] = n_frozen
        stats["rounds"] += 1
        stats["collapses"].append(n_sel)
        stats["candidates"].append(n_cand)
        if n_sel == 0:
            stats["stopped"] = "selected nothing"
            break
    V2 = F2 = 0
    if cap:
        N.check(L.nerf_decimate_count(V, F, cap, cur, N.ptr(ws), N.ptr(tot), st))
        V2, F2 = tot[:2].tolist()
        assert F2 == cap
    ov = sentinel_(torch.empty(V2 + 1, 3, dtype=torch.float32, device=DEV))
    on = sentinel_(torch.empty(V2 + 1, 3, dtype=torch.float32, device=DEV))
    oc = None if c is None else sentinel_(torch.empty(V2 + 1, 3, dtype=torch.float32, device=DEV))
    of = torch.full((F2 + 1, 3), SENT32, dtype=torch.int32, device=DEV)
    if V2:
        N.check(L.nerf_decimate_write(V, F, cur, colors, N.ptr(ws), V2, F2, N.ptr(ov), N.ptr(oc), N.ptr(of), st))
        ws2 = poison_(torch.empty(L.nerf_smooth_workspace_bytes(V2, F2), dtype=torch.uint8, device=DEV), pattern)
        N.check(L.nerf_smooth_build(V2, N.ptr(of), F2, N.ptr(ws2), st))
        N.check(L.nerf_smooth_normals(N.ptr(ov), V2, clo, chi, N.ptr(ws2), N.ptr(on), None, st))
    torch.cuda.synchronize()
    assert unwritten(ov[V2:]) == 3 and unwritten(on[V2:]) == 3 and unwritten(ov[:V2]) == 0 and unwritten(on[:V2]) == 0
    assert oc is None or (unwritten(oc[V2:]) == 3 and unwritten(oc[:V2]) == 0)
    assert bool((of[F2:] == SENT32).all())
    out = (ov[:V2].cpu().numpy(), of[:F2].cpu().numpy(), on[:V2].cpu().numpy(), None if oc is None else oc[:V2].cpu().numpy())
    return out, stats


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _assert_same(got, want, what=""):
    gv, gf, gn, gc = got
    wv, wf, wn, wc = want
    assert gv.shape == wv.shape and gf.shape == wf.shape, (what, gv.shape, wv.shape, gf.shape, wf.shape)
    assert np.array_equal(gf, wf), (what, "faces differ")
    dv = _bits(gv) != _bits(wv)
    assert not dv.any(), (what, "vertex bits differ", int(dv.sum()), gv[dv.any(1)][:4], wv[dv.any(1)][:4])
    assert np.array_equal(_bits(gn), _bits(wn)), (what, "normal bits differ")
    assert (gc is None) == (wc is None)
    if wc is not None:
        assert np.array_equal(_bits(gc), _bits(wc)), (what, "colour bits differ")


COMBOS = (("quadric", True, 4), ("quadric", False, 1), ("midpoint", True, 1), ("midpoint", False, 4))


def _targets(name):
    F = len(D.mesh(name)[1])
    return (F // 2, F // 10, 100)


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("which", (0, 1, 2))
@pytest.mark.parametrize("name", ["sphere", "box", "plate", "noise"])
def test_decimate_matches_the_reference_bit_for_bit(name, which):
    """Targets F / 2, F / 10 and 100; both placements, with and without colours, passes 1 and 4."""
    v, f, n, c = D.mesh(name)
    target = _targets(name)[which]
    for k, (placement, colors, passes) in enumerate(COMBOS):
        want, wstats, _ = D.expected(name, target, placement, colors, passes)
        got, stats = _decimate_poisoned(v, f, c if colors else None, target, placement, passes, PATTERNS[k % 2])
        print(name, target, placement, colors, passes, stats["rounds"], stats["stopped"], len(got[1]))
        assert stats == wstats, (name, target, placement, colors, passes, stats, wstats)
        _assert_same(got, want, (name, target, placement, colors, passes))


@pytest.mark.parametrize("name,target", [("sphere", 4), ("half", 4), ("half", 300), ("junk", 4), ("junk", 500)])
def test_to_the_end_open_meshes_special_values_and_bad_indices(name, target):
    """Down to a tetrahedron; a mesh with a boundary, down to what its frozen vertices allow; NaN / +-inf coordinates, indices
    outside [0, V) and a face with two equal corners."""
    v, f, n, c = D.mesh(name)
    want, wstats, _ = D.expected(name, target)
    got, stats = _decimate_poisoned(v, f, c, target, "quadric", 4)
    assert stats == wstats, (stats, wstats)
    _assert_same(got, want, (name, target))
    if name == "half":
        assert stats["frozen"] > 0 and (target > 4 or stats["stopped"] == "selected nothing")


def test_engine_decimate_stats_identity_and_frozen_mesh():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f, n, c = D.mesh("sphere")
    m = _mesh(v, f, n, c)
    out, stats = E.decimate(m, 346, D.LO, D.HI)
    want, wstats, _ = D.expected("sphere", 346)
    assert isinstance(stats, E.DecimateStats) and stats._asdict() == wstats
    _assert_same((out.verts.cpu().numpy(), out.faces.cpu().numpy(), out.normals.cpu().numpy(), out.colors.cpu().numpy()), want)
    # twice: the same bits
    again, _ = E.decimate(m, 346, D.LO, D.HI)
    assert bits_equal(again.verts, out.verts) and torch.equal(again.faces, out.faces) and bits_equal(again.colors, out.colors)
    # max_rounds
    part, pstats = E.decimate(m, 346, D.LO, D.HI, max_rounds=2)
    assert pstats.rounds == 2 and pstats.stopped == "max_rounds" and pstats.collapses == wstats["collapses"][:2]
    assert part.faces.shape[0] == len(f) - 2 * sum(pstats.collapses)
    # target >= F: the input itself
    for t in (len(f), len(f) + 1, 10 ** 9):
        same, s0 = E.decimate(m, t, D.LO, D.HI)
        assert same is m and s0 == E.DecimateStats(0, [], [], 0, "target")
    # a strip two vertices wide: every vertex lies on the boundary
    k = 20
    sv = np.array([[0.04 * i - 0.4, 0.1 * j, 0.0] for i in range(k) for j in range(2)], np.float32)
    sf = np.array([t for i in range(k - 1) for t in ((2 * i, 2 * i + 2, 2 * i + 1), (2 * i + 1, 2 * i + 2, 2 * i + 3))], np.int32)
    sm = _mesh(sv, sf, np.zeros_like(sv), None)
    out, stats = E.decimate(sm, 4, D.LO, D.HI)
    assert stats == E.DecimateStats(1, [0], [0], 2 * k, "selected nothing")
    assert bits_equal(out.verts, sm.verts) and torch.equal(out.faces, sm.faces) and out.colors is None
    want, wstats = D.decimate(sv, sf, np.zeros_like(sv), None, 4)
    assert wstats == stats._asdict() and np.array_equal(_bits(out.normals.cpu().numpy()), _bits(want[2]))


def test_the_sphere_at_128_against_the_reference():
    """55 612 faces to a tenth: more than one scan block of faces, edges and vertices.  The reference takes about two seconds, so
    the bits are compared and not the invariants alone."""
    v, f, n, c = D.mesh("big")
    target = len(f) // 10
    want, wstats, _ = D.expected("big", target)
    got, stats = _decimate_poisoned(v, f, c, target, "quadric", 4)
    print(len(f), "->", len(got[1]), stats["rounds"], stats["collapses"])
    assert stats == wstats
    _assert_same(got, want, "big")
    assert len(got[1]) in (target, target - 1) and D.euler(got[1]) == 2 and D.all_edges_paired(got[1])


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_return_before_any_device_work():
    from nerf_meets_mlx_amd import _native as N
    from nerf_meets_mlx_amd.engine import mesh as E
    L, st = N.lib(), N.stream()
    v, f, n, c = D.mesh("box")
    m = _mesh(v, f, n, c)
    V, F = len(v), len(f)
    for bad in ({"mesh": (m.verts, m.faces)}, {"target_faces": 3}, {"target_faces": 100.0}, {"target_faces": True}, {"passes": 0},
                {"passes": 17}, {"passes": 2.0}, {"max_rounds": 0}, {"lo": [1.0, -1.0, -1.0]}, {"hi": [float("nan"), 1.0, 1.0]},
                {"placement": "mean"}, {"placement": 1}, {"mesh": E.Mesh(m.verts, m.faces.long(), m.normals, None)}):
        kw = {"mesh": m, "target_faces": 100, "lo": D.LO, "hi": D.HI, **bad}
        with pytest.raises(ValueError):
            E.decimate(**kw)
        with pytest.raises(ValueError):
            E.check_decimate_args(**kw)
    lo, hi = (C.c_float * 3)(*D.LO), (C.c_float * 3)(*D.HI)
    flat = (C.c_float * 3)(1.0, -1.0, -1.0)
    ws = poison_(torch.empty(L.nerf_decimate_workspace_bytes(V, F), dtype=torch.uint8, device=DEV), NAN_BYTES)
    keys = torch.full((6 * F,), -7, dtype=torch.int64, device=DEV)
    tot = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    ov = sentinel_(torch.empty(V, 3, dtype=torch.float32, device=DEV))
    of = torch.full((F, 3), SENT32, dtype=torch.int32, device=DEV)
    big = (1 << 24) + 1
    p = N.ptr
    assert L.nerf_decimate_begin(p(m.verts), None, big, p(m.faces), F, p(ws), p(tot), st) == E_SHAPE
    assert L.nerf_decimate_begin(p(m.verts), None, V, p(m.faces), 0, p(ws), p(tot), st) == E_SHAPE
    assert L.nerf_decimate_begin(None, None, V, p(m.faces), F, p(ws), p(tot), st) == E_NULL
    assert L.nerf_decimate_begin(p(m.verts), None, V, p(m.faces), F, None, p(tot), st) == E_NULL
    assert L.nerf_decimate_keys(V, F, F + 1, 0, p(ws), p(keys), st) == E_SHAPE
    assert L.nerf_decimate_keys(V, F, F, 2, p(ws), p(keys), st) == E_SHAPE
    assert L.nerf_decimate_keys(V, F, F, 0, p(ws), None, st) == E_NULL
    assert L.nerf_decimate_edges(V, F, 0, p(keys), p(ws), st) == E_SHAPE
    assert L.nerf_decimate_edges(V, F, F, None, p(ws), st) == E_NULL
    assert L.nerf_decimate_quadrics(V, F, 0, flat, hi, p(ws), st) == E_SHAPE
    assert L.nerf_decimate_quadrics(V, F, 0, None, hi, p(ws), st) == E_NULL
    for passes, code in ((0, 1), (17, 1), (4, 2), (4, -1)):
        assert L.nerf_decimate_select(V, F, F, 0, lo, hi, code, passes, p(ws), p(keys), st) == E_SHAPE
    assert L.nerf_decimate_select(V, F, F, 0, lo, hi, 1, 4, p(ws), None, st) == E_NULL
    assert L.nerf_decimate_apply(V, F, F, 0, lo, hi, 1, 0, -1, p(keys), p(ws), p(tot), st) == E_SHAPE
    assert L.nerf_decimate_apply(V, F, F, 0, lo, flat, 1, 0, 100, p(keys), p(ws), p(tot), st) == E_SHAPE
    assert L.nerf_decimate_apply(V, F, F, 0, lo, hi, 1, 0, 100, None, p(ws), p(tot), st) == E_NULL
    assert L.nerf_decimate_count(V, F, F, 0, p(ws), None, st) == E_NULL
    assert L.nerf_decimate_count(-1, F, F, 0, p(ws), p(tot), st) == E_SHAPE
    assert L.nerf_decimate_write(V, F, 0, 0, p(ws), V + 1, 1, p(ov), None, p(of), st) == E_SHAPE
    assert L.nerf_decimate_write(V, F, 0, 0, p(ws), 1, F + 1, p(ov), None, p(of), st) == E_SHAPE
    assert L.nerf_decimate_write(V, F, 0, 0, p(ws), 1, 1, p(ov), p(ov), p(of), st) == E_SHAPE
    assert L.nerf_decimate_write(V, F, 0, 0, p(ws), 1, 1, None, None, p(of), st) == E_NULL
    assert b"nerf_decimate_write" in L.nerf_last_error()
    for bad in ((0, 8), (8, 0), (big, 8), (8, big)):
        assert L.nerf_decimate_workspace_bytes(*bad) == -1
    torch.cuda.synchronize()
    assert bool((keys == -7).all()) and bool((tot == -7).all()) and bool((of == SENT32).all()) and unwritten(ov) == ov.numel()
    assert bool((ws == NAN_BYTES).all())


# ------------------------------------------------------------------------------------------------ the trainer's hook
def test_trainer_decimate_mesh():
    """Trainer.decimate_mesh is engine.mesh.decimate on the trainer's box; no training step is needed for that."""
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine import mesh as E
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    imgs, poses, _, _, K = synthetic.make_dataset(16, 16, 2, seed=0, device=DEV)
    tr = NGPTrainer(imgs, poses, K, N_rand=64, n_depth_samples=16, seed=4, device=DEV, log2_hashmap_size=10)
    v, f, n, c = D.mesh("box")
    m = _mesh(v, f, n, c)
    out, stats = tr.decimate_mesh(m, 200, placement="midpoint")
    lo, hi = tr._mesh_box(None)
    want, wstats = E.decimate(m, 200, lo, hi, placement="midpoint")
    assert stats == wstats and out.faces.shape[0] in (199, 200)
    assert bits_equal(out.verts, want.verts) and torch.equal(out.faces, want.faces) and bits_equal(out.colors, want.colors)
    ref, rstats = D.decimate(v, f, n, c, 200, lo, hi, "midpoint")
    assert rstats == stats._asdict() and np.array_equal(_bits(out.verts.cpu().numpy()), _bits(ref[0]))
    box, bstats = tr.decimate_mesh(m, 200, aabb=(D.LO, D.HI))
    _assert_same((box.verts.cpu().numpy(), box.faces.cpu().numpy(), box.normals.cpu().numpy(), box.colors.cpu().numpy()),
                 D.expected("box", 200)[0])
    with pytest.raises(ValueError):
        tr.decimate_mesh(m, 3)
