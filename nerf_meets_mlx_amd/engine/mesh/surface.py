"""The surface stage: what runs on a marching-cubes mesh before it is coloured (include/nerf_hip.h "mesh simplification", "mesh
smoothing"; DESIGN.md sections 27, 30).

  * `simplify(mesh, grid, lo, hi, placement)` decimates a mesh by vertex clustering on a `grid`^3 lattice of the box, one vertex
    per occupied cell placed by the cell's quadric (box corners and edges survive) or at the mean; opposite faces that land on
    the same three cells annihilate, so one-voxel-thick sheets vanish.  `extract(..., simplify_grid, simplify_placement)` runs
    it between marching cubes and the colour query.
  * `smooth(mesh, iterations, lo, hi, lam, mu)` moves the vertices by `iterations` pairs of Taubin's lambda|mu umbrella steps
    (mu = 0: plain Laplacian) and recomputes the normals from the faces; the faces and the colours are the input's.
    `extract(..., smooth_iterations, smooth_lambda, smooth_mu)` runs it between marching cubes and the simplifier.
  * `check_surface_options` is the one check of those five keywords for `extract` and the trainers."""
import math
from typing import Sequence

import torch

from ... import _native as N
from ._base import MAX_RES, Mesh, _box, _check_mesh_tensors, _mark, check_mesh_args
from ._checks import f32, is_int, is_number, need_int

PLACEMENTS = {"mean": 0, "quadric": 1}   # NERF_SIMPLIFY_MEAN / NERF_SIMPLIFY_QUADRIC
SIMPLIFY_MAX_CLUSTERS = 1 << 21
SMOOTH_MAX_ITERATIONS = 1024


def check_simplify_grid(grid) -> int:
    """simplify_grid as an int; ValueError for a bool, a non-integral value or one outside {0} + [2, MAX_RES] (0: no
    simplification)."""
    if not (is_int(grid, 0, 0) or is_int(grid, 2, MAX_RES)):
        raise ValueError(f"simplify_grid must be 0 or an int in [2, {MAX_RES}], got {grid!r}")
    return int(grid)


def _check_placement(placement) -> int:
    if not isinstance(placement, str) or placement not in PLACEMENTS:
        raise ValueError(f"simplify placement must be one of {sorted(PLACEMENTS)}, got {placement!r}")
    return PLACEMENTS[placement]


def check_simplify_args(mesh, grid, lo: Sequence[float], hi: Sequence[float], placement="quadric"):
    """(grid, lo [3], hi [3], placement code) as (int, float lists, int); ValueError for a grid that is not an int in
    [2, MAX_RES], a placement other than "mean" / "quadric", a box with lo >= hi or a non-finite corner, or a mesh whose tensors
    are not contiguous verts float32 [V, 3], faces int32 [F, 3], normals float32 [V, 3] and colors None or float32 [V, 3] on one
    device, with V, F <= 2^24 and min(V, grid^3) <= 2^21."""
    if check_simplify_grid(grid) < 2:
        raise ValueError(f"simplify grid must be an int in [2, {MAX_RES}], got {grid!r}")
    grid, lo, hi, _ = check_mesh_args(int(grid), lo, hi)
    code = _check_placement(placement)
    V, F = _check_mesh_tensors("simplify", mesh)
    if min(V, grid ** 3) > SIMPLIFY_MAX_CLUSTERS:
        raise ValueError(f"simplify: min(V, grid^3) = {min(V, grid ** 3)} possible clusters exceed 2^21; use a coarser grid")
    return grid, lo, hi, code


def _simplify(mesh: Mesh, grid, lo, hi, placement, color_rows: bool, mark=None):
    """(Mesh, colour rows or None, clusters before the unused ones go).  mark: _mark's hook ("cluster", "sort", "count" -- it
    ends behind the host read --, "write")."""
    G, lo, hi, code = check_simplify_args(mesh, grid, lo, hi, placement)
    dev = mesh.verts.device
    V, F = mesh.verts.shape[0], mesh.faces.shape[0]
    L = N.lib()
    clo, chi = _box(lo, hi)
    ws = torch.empty(L.nerf_simplify_workspace_bytes(V, F, G), dtype=torch.uint8, device=dev)
    keys = torch.empty(F, dtype=torch.int64, device=dev)
    tot = torch.empty(3, dtype=torch.int64, device=dev)
    _mark(mark, "cluster")
    N.check(L.nerf_simplify_cluster(N.ptr(mesh.verts), N.ptr(mesh.normals), N.ptr(mesh.colors), V, N.ptr(mesh.faces), F, clo, chi,
                                    G, N.ptr(ws), N.ptr(keys), N.stream()))
    _mark(mark, "sort")
    skeys, perm = torch.sort(keys, stable=True)               # plumbing between two of our launches: groups faces by vertex set
    _mark(mark, "count")
    N.check(L.nerf_simplify_count(N.ptr(skeys), N.ptr(perm), V, N.ptr(mesh.faces), F, G, N.ptr(ws), N.ptr(tot), N.stream()))
    V2, F2, K = tot.tolist()                                  # the one host read
    _mark(mark, "write")
    verts = torch.empty(V2, 3, dtype=torch.float32, device=dev)
    normals = torch.empty(V2, 3, dtype=torch.float32, device=dev)
    colors = torch.empty(V2, 3, dtype=torch.float32, device=dev) if mesh.colors is not None else None
    rows = torch.empty(V2, 11, dtype=torch.float32, device=dev) if color_rows else None
    faces = torch.empty(F2, 3, dtype=torch.int32, device=dev)
    if V2 or F2:
        N.check(L.nerf_simplify_write(V, N.ptr(mesh.faces), F, clo, chi, G, code, N.ptr(ws), V2, F2, N.ptr(verts), N.ptr(normals),
                                      N.ptr(colors), N.ptr(rows), N.ptr(faces), N.stream()))
    return Mesh(verts, faces, normals, colors), rows, K


def simplify(mesh: Mesh, grid: int, lo, hi, placement: str = "quadric") -> Mesh:
    """The mesh clustered on the `grid`^3 cells of the box [lo, hi]: one vertex per occupied cell that a surviving face uses, at
    the minimiser of the cell's area^2-weighted plane quadric pulled slightly towards the mean ("quadric") or at the mean of the
    cell's vertices ("mean"); normals are the normalised sums, colours (when the input has them, else None) the means.  Faces
    with two corners in one cell go, and faces of opposite orientation on the same three cells cancel in pairs
    (nerf_simplify_cluster, a stable torch.sort of the face keys, nerf_simplify_count, one read of (V', F') to the host,
    nerf_simplify_write).  Bit-reproducible and independent of the order of the input's vertices and faces."""
    return _simplify(mesh, grid, lo, hi, placement, False)[0]


def check_smooth_params(iterations, lam=0.5, mu=-0.53):
    """(iterations, lam, mu) as (int, float, float), lam and mu rounded to float32 as the library receives them; ValueError for
    an iterations that is a bool, non-integral or outside [0, SMOOTH_MAX_ITERATIONS] (0: no smoothing), a lam outside (0, 1], a
    mu that is neither 0 nor in [-2, 0), or either being a bool, not a real number or NaN."""
    iterations = need_int(iterations, "smooth iterations", 0, SMOOTH_MAX_ITERATIONS)
    for name, x in (("lambda", lam), ("mu", mu)):
        if not is_number(x) or math.isnan(float(x)):
            raise ValueError(f"smooth {name} must be a number, got {x!r}")
    lam, mu = f32(lam), f32(mu)
    if not 0.0 < lam <= 1.0:
        raise ValueError(f"smooth lambda must be in (0, 1] as a float32, got {lam!r}")
    if not (mu == 0.0 or -2.0 <= mu < 0.0):
        raise ValueError(f"smooth mu must be 0 (plain Laplacian) or in [-2, 0), got {mu!r}")
    return iterations, lam, mu


def check_smooth_args(mesh, iterations, lo: Sequence[float], hi: Sequence[float], lam=0.5, mu=-0.53):
    """(iterations, lo [3], hi [3], lam, mu) as (int, float lists, floats); ValueError for an iterations that is not an int in
    [1, SMOOTH_MAX_ITERATIONS], a lam outside (0, 1], a mu that is neither 0 nor in [-2, 0) (bools, non-numbers and NaN are
    refused), a box with lo >= hi or a non-finite corner, or a mesh whose tensors are not contiguous verts float32 [V, 3], faces
    int32 [F, 3], normals float32 [V, 3] and colors None or float32 [V, 3] on one device, with V, F <= 2^24."""
    iterations, lam, mu = check_smooth_params(iterations, lam, mu)
    need_int(iterations, "smooth iterations", 1, SMOOTH_MAX_ITERATIONS)
    _, lo, hi, _ = check_mesh_args(2, lo, hi)
    _check_mesh_tensors("smooth", mesh)
    return iterations, lo, hi, lam, mu


def _smooth(mesh: Mesh, iterations, lo, hi, lam, mu, color_rows: bool, mark=None):
    """(Mesh, colour rows or None).  mark: _mark's hook ("build", "run", "normals")."""
    iterations, lo, hi, lam, mu = check_smooth_args(mesh, iterations, lo, hi, lam, mu)
    dev = mesh.verts.device
    V, F = mesh.verts.shape[0], mesh.faces.shape[0]
    L = N.lib()
    clo, chi = _box(lo, hi)
    verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
    normals = torch.empty(V, 3, dtype=torch.float32, device=dev)
    rows = torch.empty(V, 11, dtype=torch.float32, device=dev) if color_rows else None
    if V:
        ws = torch.empty(L.nerf_smooth_workspace_bytes(V, F), dtype=torch.uint8, device=dev)
        _mark(mark, "build")
        N.check(L.nerf_smooth_build(V, N.ptr(mesh.faces), F, N.ptr(ws), N.stream()))
        _mark(mark, "run")
        N.check(L.nerf_smooth_run(N.ptr(mesh.verts), V, clo, chi, iterations, lam, mu, N.ptr(ws), N.ptr(verts), N.stream()))
        _mark(mark, "normals")
        N.check(L.nerf_smooth_normals(N.ptr(verts), V, clo, chi, N.ptr(ws), N.ptr(normals), N.ptr(rows), N.stream()))
    return Mesh(verts, mesh.faces, normals, mesh.colors), rows


def smooth(mesh: Mesh, iterations: int, lo, hi, lam: float = 0.5, mu: float = -0.53) -> Mesh:
    """The mesh after `iterations` pairs of Taubin's lambda|mu filter: an umbrella-Laplacian half-step with factor `lam`, then
    one with `mu` (< -lam keeps the volume; mu = 0 is plain Laplacian smoothing and launches no second half-step).  A
    neighbour weighs as many times as faces share the edge; the box [lo, hi] only fixes the fixed-point scale of the exact
    sums.  Same `faces` tensor, new `verts`, new `normals` (area-weighted from the faces), `colors` carried over: vertices
    keep their identity (nerf_smooth_build, nerf_smooth_run, nerf_smooth_normals; no host read).  Bit-reproducible and
    independent of the order of the faces."""
    return _smooth(mesh, iterations, lo, hi, lam, mu, False)[0]


def check_surface_options(simplify_grid, simplify_placement, smooth_iterations, smooth_lambda, smooth_mu):
    """(simplify_grid, simplify_placement, smooth_iterations, smooth_lambda, smooth_mu) as (int, str, int, float, float), as
    mesh_volume takes them: the surface-stage keywords of extract, Trainer.extract_mesh and NGPTrainer.extract_mesh_tsdf, checked
    in this order by check_simplify_grid, the placement's refusal and check_smooth_params."""
    simplify_grid = check_simplify_grid(simplify_grid)
    _check_placement(simplify_placement)
    return (simplify_grid, simplify_placement, *check_smooth_params(smooth_iterations, smooth_lambda, smooth_mu))
