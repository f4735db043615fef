"""Decimation to a target face count (include/nerf_hip.h "edge-collapse decimation").

  * `decimate(mesh, target_faces, lo, hi, placement, passes, max_rounds)` collapses edges greedily by quadric error, an
    independent set of them per round, until the mesh has `target_faces` faces (or one fewer: a collapse removes two).  What
    `simplify` cannot do: there the output size follows from the grid alone.  Returns the mesh and a `DecimateStats`.
  * `check_decimate_args` is the one check of its arguments, before any device work."""
from typing import List, NamedTuple, Sequence

import torch

from ... import _native as N
from ._base import Mesh, _box, _check_mesh_tensors, _mark, check_mesh_args
from ._checks import is_int, need_int

DECIMATE_PLACEMENTS = {"midpoint": 0, "quadric": 1}   # NERF_DECIMATE_MIDPOINT / NERF_DECIMATE_QUADRIC
DECIMATE_MAX_PASSES = 16
DECIMATE_MAX_ROUNDS = 1 << 20
DECIMATE_STOPS = ("target", "selected nothing", "max_rounds")


class DecimateStats(NamedTuple):
    rounds: int                 # rounds run (the one that selected nothing included)
    collapses: List[int]        # per round
    candidates: List[int]       # per round
    frozen: int                 # vertices on an edge that the first round could not move (open, non-manifold, not finite)
    stopped: str                # one of DECIMATE_STOPS


def check_decimate_args(mesh, target_faces, lo: Sequence[float], hi: Sequence[float], placement="quadric", passes=4, max_rounds=1024):
    """(target_faces, lo [3], hi [3], placement code, passes, max_rounds) as (int, float lists, int, int, int); ValueError for a
    mesh that is not a Mesh of contiguous verts float32 [V, 3], faces int32 [F, 3], normals float32 [V, 3] and colors None or
    float32 [V, 3] on one device with V, F <= 2^24, a target_faces that is not an int >= 4, a passes outside
    [1, DECIMATE_MAX_PASSES], a max_rounds outside [1, DECIMATE_MAX_ROUNDS], a box with lo >= hi or a non-finite corner, or a
    placement other than "midpoint" / "quadric"."""
    _check_mesh_tensors("decimate", mesh)
    if not is_int(target_faces, 4, 1 << 62):
        raise ValueError(f"decimate: target_faces must be an int >= 4, got {target_faces!r}")
    passes = need_int(passes, "decimate passes", 1, DECIMATE_MAX_PASSES)
    max_rounds = need_int(max_rounds, "decimate max_rounds", 1, DECIMATE_MAX_ROUNDS)
    _, lo, hi, _ = check_mesh_args(2, lo, hi)
    if not isinstance(placement, str) or placement not in DECIMATE_PLACEMENTS:
        raise ValueError(f"decimate placement must be one of {sorted(DECIMATE_PLACEMENTS)}, got {placement!r}")
    return int(target_faces), lo, hi, DECIMATE_PLACEMENTS[placement], passes, max_rounds


def _decimate(mesh: Mesh, target_faces, lo, hi, placement="quadric", passes=4, max_rounds=1024, mark=None):
    """(Mesh, DecimateStats).  mark: _mark's hook ("begin", then per round "keys", "sort", "edges", "select", "trim sort", "apply"
    -- it ends behind the round's host read --, then "finish", "normals")."""
    target, lo, hi, code, passes, max_rounds = check_decimate_args(mesh, target_faces, lo, hi, placement, passes, max_rounds)
    V, F = mesh.verts.shape[0], mesh.faces.shape[0]
    if target >= F:
        return mesh, DecimateStats(0, [], [], 0, "target")
    if V == 0:                                           # no face has a valid corner
        return Mesh(mesh.verts, mesh.faces[:0], mesh.normals, mesh.colors), DecimateStats(0, [], [], 0, "target")
    dev = mesh.verts.device
    L, st = N.lib(), N.stream()
    clo, chi = _box(lo, hi)
    has_colors = int(mesh.colors is not None)
    ws = torch.empty(L.nerf_decimate_workspace_bytes(V, F), dtype=torch.uint8, device=dev)
    keys = torch.empty(2 * 3 * F, dtype=torch.int64, device=dev)
    sel_keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
    tot = torch.empty(4, dtype=torch.int64, device=dev)
    _mark(mark, "begin")
    N.check(L.nerf_decimate_begin(N.ptr(mesh.verts), N.ptr(mesh.colors), V, N.ptr(mesh.faces), F, N.ptr(ws), N.ptr(tot), st))
    cap, cur = int(tot[0]), 0                            # the faces with three valid, distinct corners: read once
    rounds, collapses, candidates, frozen, stopped = 0, [], [], 0, DECIMATE_STOPS[0]
    while cap > target:
        if rounds == max_rounds:
            stopped = DECIMATE_STOPS[2]
            break
        k, s = keys[:6 * cap].view(2, 3 * cap), sel_keys[:3 * cap]
        _mark(mark, "keys")
        N.check(L.nerf_decimate_keys(V, F, cap, cur, N.ptr(ws), N.ptr(k), st))
        _mark(mark, "sort")
        sk = torch.sort(k, dim=1).values                 # plumbing between two of our launches: edges and vertex rows
        _mark(mark, "edges")
        N.check(L.nerf_decimate_edges(V, F, cap, N.ptr(sk), N.ptr(ws), st))
        if rounds == 0:
            N.check(L.nerf_decimate_quadrics(V, F, cur, clo, chi, N.ptr(ws), st))
        _mark(mark, "select")
        N.check(L.nerf_decimate_select(V, F, cap, cur, clo, chi, code, passes, N.ptr(ws), N.ptr(s), st))
        _mark(mark, "trim sort")
        ss = torch.sort(s).values                        # the k smallest selected keys, should the round overshoot
        _mark(mark, "apply")
        N.check(L.nerf_decimate_apply(V, F, cap, cur, clo, chi, code, has_colors, target, N.ptr(ss), N.ptr(ws), N.ptr(tot), st))
        cap, n_sel, n_cand, n_frozen = tot.tolist()      # the round's one host read
        cur = 1 - cur
        if rounds == 0:
            frozen = n_frozen
        rounds += 1
        collapses.append(n_sel)
        candidates.append(n_cand)
        if n_sel == 0:
            stopped = DECIMATE_STOPS[1]
            break
    _mark(mark, "finish")
    if cap:
        N.check(L.nerf_decimate_count(V, F, cap, cur, N.ptr(ws), N.ptr(tot), st))
        V2, F2 = tot[:2].tolist()
    else:
        V2 = F2 = 0
    verts = torch.empty(V2, 3, dtype=torch.float32, device=dev)
    normals = torch.empty(V2, 3, dtype=torch.float32, device=dev)
    colors = torch.empty(V2, 3, dtype=torch.float32, device=dev) if has_colors else None
    faces = torch.empty(F2, 3, dtype=torch.int32, device=dev)
    if V2:
        N.check(L.nerf_decimate_write(V, F, cur, has_colors, N.ptr(ws), V2, F2, N.ptr(verts), N.ptr(colors), N.ptr(faces), st))
        _mark(mark, "normals")                           # the smoothing stage's rule and code
        ws2 = torch.empty(L.nerf_smooth_workspace_bytes(V2, F2), dtype=torch.uint8, device=dev)
        N.check(L.nerf_smooth_build(V2, N.ptr(faces), F2, N.ptr(ws2), st))
        N.check(L.nerf_smooth_normals(N.ptr(verts), V2, clo, chi, N.ptr(ws2), N.ptr(normals), None, st))
    return Mesh(verts, faces, normals, colors), DecimateStats(rounds, collapses, candidates, frozen, stopped)


def decimate(mesh: Mesh, target_faces: int, lo, hi, placement: str = "quadric", passes: int = 4, max_rounds: int = 1024):
    """(Mesh, DecimateStats): the mesh collapsed to `target_faces` faces (or one fewer) by greedy quadric-error edge collapse.
    Per round every edge whose ends are both interior manifold vertices, whose link condition holds and whose collapse flips no
    face is a candidate with the cost of its merged quadric at its new position -- the regularised minimiser of that quadric
    ("quadric") or the midpoint ("midpoint") --, `passes` passes pick edges that are the cheapest within two rings, and all of
    them collapse at once.  Vertices on open or non-manifold edges are never moved, so a target below what the free vertices
    allow stops with "selected nothing".  Normals are recomputed from the faces, colours are the means of the merged vertices.
    `target_faces >= F` returns the input mesh itself.  Deterministic, bit-reproducible; the result depends on the order of the
    faces (the initial quadrics are fixed-order double sums)."""
    return _decimate(mesh, target_faces, lo, hi, placement, passes, max_rounds)
