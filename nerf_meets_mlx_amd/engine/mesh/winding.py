"""The winding stage: on which side of a mesh a point lies (include/nerf_hip.h "mesh winding number").  The
generalized winding number is 1 inside a closed mesh whose faces are counter-clockwise seen from outside, 0 outside, and in
between near a hole; it is defined for open, duplicated and self-intersecting meshes.  It changes no mesh.

  * `MeshWinding(mesh, lo, hi, bvh)` adds one float64 record of moments per node to a `MeshBVH` (its own, or the caller's);
    `.query(points, beta)` answers, per point, the winding number w and (faces evaluated exactly, nodes replaced by their dipole).
    A subtree is replaced when the point is more than `beta` radii from its centre; `beta=inf` is the exact sum.
    `winding_number` is the one-shot form.
  * `winding_volume(mesh, resolution, lo, hi, beta)` is w on the lattice of the box, float32 [R, R, R].
  * `remesh(mesh, resolution, lo, hi, ...)` is marching cubes of that volume at 0.5, behind the volume stage's filters: a closed
    mesh from one with holes.
  * `signed_distance(points, mesh, lo, hi, beta, index)` gives the distance query's answer the sign of w > 0.5.
  * `check_winding_args` is the one check of their arguments."""
import math
from typing import Optional

import torch

from ... import _native as N
from ._base import CHUNK, Mesh, _check_mesh_tensors, _clamped, _mark, _query_in_order, check_mesh_args
from ._checks import is_number, need_tensor
from .distance import BVH_SORTED_QUERY, DISTANCE_MAX_SAMPLES, MeshBVH, _index, _morton_order, check_distance_index
from .volume import _rows_into, check_volume_options, filter_volume, marching_cubes

WINDING_NODE_DOUBLES = 12         # N [0:3], c [3:6], r [6], A [7], S [8:11], 0
WINDING_INSIDE = 0.5              # inside is w > 0.5


def check_winding_args(mesh, lo, hi, beta=2.0, resolution=2, points=None):
    """(beta, lo [3], hi [3], resolution) as (float, float lists, int); ValueError for a beta that is a bool, not a number, NaN
    or below 1 (+inf is the exact sum), a resolution (of those that take one) that is no int in [2, MAX_RES], a box with lo >= hi or a
    non-finite corner, a mesh whose tensors are not contiguous verts float32 [V, 3], faces int32 [F, 3], normals float32 [V, 3] and
    colors None or float32 [V, 3] on one device with V, F <= 2^24, or `points` that are not None and not a contiguous float32
    [n, 3] tensor of at most 2^30 rows on the mesh's device."""
    if not is_number(beta) or math.isnan(float(beta)) or float(beta) < 1.0:
        raise ValueError(f"winding beta must be a number >= 1 or +inf, got {beta!r}")
    R, lo, hi, _ = check_mesh_args(resolution, lo, hi)
    _check_mesh_tensors("winding", mesh)
    if points is not None:
        need_tensor(points, "winding: points", torch.float32, (None, 3), mesh.verts.device, "[n, 3]")
        if points.shape[0] > DISTANCE_MAX_SAMPLES:
            raise ValueError(f"winding: at most 2^30 points, got {points.shape[0]}")
    return float(beta), lo, hi, R


class MeshWinding:
    """The moments of `mesh` on a face hierarchy: `bvh` (a MeshBVH of this very mesh) or a new MeshBVH(mesh, lo, hi), then per
    node the sum of the faces' area vectors, their area-weighted centroid and the radius of the node's box about it
    (nerf_winding_build: no host read).  The box only shapes the tree.  The mesh's tensors must not change while it is in use.
    mark: _mark's hook (the MeshBVH's stages when it is built here, then "moments")."""

    def __init__(self, mesh: Mesh, lo, hi, bvh: Optional[MeshBVH] = None, mark=None):
        _, lo, hi, _ = check_winding_args(mesh, lo, hi)
        if bvh is None:
            bvh = MeshBVH(mesh, lo, hi, mark)
        elif not isinstance(bvh, MeshBVH) or bvh.mesh.verts is not mesh.verts or bvh.mesh.faces is not mesh.faces:
            raise ValueError("winding: bvh must be a MeshBVH of this mesh")
        self.mesh, self.lo, self.hi, self.bvh = mesh, lo, hi, bvh
        self.V, self.F, self.P = bvh.V, bvh.F, bvh.P
        L = N.lib()
        size = L.nerf_winding_workspace_bytes(self.F)
        # without a face nothing is launched: the records are the zeros of an empty node
        self._ws = (torch.empty if self.F else torch.zeros)(size, dtype=torch.uint8, device=mesh.verts.device)
        _mark(mark, "moments")
        N.check(L.nerf_winding_build(N.ptr(mesh.verts), self.V, N.ptr(mesh.faces), self.F, N.ptr(bvh._ws), N.ptr(self._ws), N.stream()))

    @property
    def moments(self):
        """float64 [2 P, 12]: node i in heap order as N [0:3], c [3:6], r [6], A [7], S [8:11], 0.  A view: do not write."""
        return self._ws[:2 * self.P * WINDING_NODE_DOUBLES * 8].view(torch.float64).view(2 * self.P, WINDING_NODE_DOUBLES)

    def query(self, points: torch.Tensor, beta=2.0, sort: Optional[bool] = None, mark=None):
        """(w float64 [n], visits int32 [n, 2]) of points [n, 3]: the winding number, and (faces evaluated exactly, nodes replaced
        by their dipole); (NaN, 0, 0) for a point with a non-finite coordinate, (0, 0, 0) when the mesh has no valid face
        (nerf_winding_query: no host read, any number of calls per build).  `sort` as in MeshBVH.query: the points in their Morton
        order, the same bits back (None: BVH_SORTED_QUERY).  mark: _mark's hook ("sort", "query", "scatter")."""
        beta, _, _, _ = check_winding_args(self.mesh, self.lo, self.hi, beta, points=points)
        n, dev = points.shape[0], points.device
        outs = (torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, 2, dtype=torch.int32, device=dev))
        sort = BVH_SORTED_QUERY if sort is None else bool(sort)
        return _query_in_order(points, _morton_order(self.lo, self.hi) if sort else None, outs, lambda p, w, visits: N.check(
            N.lib().nerf_winding_query(N.ptr(p), n, N.ptr(self.mesh.verts), self.V, N.ptr(self.mesh.faces), self.F, N.ptr(self.bvh._ws),
                                       N.ptr(self._ws), beta, N.ptr(w), N.ptr(visits), N.stream())), mark)


def winding_number(points: torch.Tensor, mesh: Mesh, lo, hi, beta=2.0):
    """MeshWinding(mesh, lo, hi).query(points, beta)."""
    check_winding_args(mesh, lo, hi, beta, points=points)
    return MeshWinding(mesh, lo, hi).query(points, beta)


def _winding_volume(winding: MeshWinding, R: int, beta: float, chunk: int = CHUNK, mark=None):
    """(float32 [R, R, R], the sum of visits int64 [2]) of a built MeshWinding on the lattice of its box, `chunk` points a query."""
    dev = winding.mesh.verts.device
    n3 = R ** 3
    vol = torch.empty(n3, dtype=torch.float32, device=dev)
    total = torch.zeros(2, dtype=torch.int64, device=dev)
    chunk = _clamped(chunk, n3)
    rays = torch.empty(chunk, 11, dtype=torch.float32, device=dev)
    z = torch.empty(chunk, 1, dtype=torch.float32, device=dev)
    _mark(mark, "volume")
    for p0 in range(0, n3, chunk):
        cnt = min(chunk, n3 - p0)
        _rows_into(R, winding.lo, winding.hi, p0, cnt, rays[:cnt], z[:cnt])
        w, visits = winding.query(rays[:cnt, :3].contiguous(), beta, sort=False)       # the lattice order is coherent already
        vol[p0:p0 + cnt] = w.float()                                                   # rounded once
        total += visits.sum(0)
    return vol.view(R, R, R), total


def winding_volume(mesh: Mesh, resolution: int, lo, hi, beta=2.0) -> torch.Tensor:
    """float32 [R, R, R]: the winding number of `mesh` at the lattice points of the box [lo, hi] (vol[k, j, i] at the cell centres
    lo + (i + 0.5) h, nerf_mesh_points), CHUNK points a query, each value w rounded once to float32.  It does not depend on the
    chunking."""
    beta, lo, hi, R = check_winding_args(mesh, lo, hi, beta, resolution)
    return _winding_volume(MeshWinding(mesh, lo, hi), R, beta)[0]


def remesh(mesh: Mesh, resolution: int, lo, hi, beta=2.0, min_component: int = 0, largest_only: bool = False,
           opening_radius: int = 0) -> Mesh:
    """marching_cubes(filter_volume(winding_volume(mesh, resolution, lo, hi, beta), 0.5, ...), 0.5, lo, hi): the surface
    {w = 0.5} of a mesh that may be open, duplicated or self-intersecting, closed wherever it stays inside the box, with the volume
    stage's filters (`min_component`, `largest_only`, `opening_radius` as in extract).  No colours: vertex_colors, bake_texture or
    project_texture colour the result."""
    beta, lo, hi, R = check_winding_args(mesh, lo, hi, beta, resolution)
    options = check_volume_options(min_component, largest_only, opening_radius, R)
    vol = _winding_volume(MeshWinding(mesh, lo, hi), R, beta)[0]
    return marching_cubes(filter_volume(vol, WINDING_INSIDE, *options), WINDING_INSIDE, lo, hi)


def signed_distance(points: torch.Tensor, mesh: Mesh, lo, hi, beta=2.0, index="bvh"):
    """(sd float32 [n], face int32 [n], w float64 [n]) of points [n, 3]: |sd| is the square root (torch float64, rounded once to
    float32) of the dist2 that point_mesh_distance(points, mesh, lo, hi, index=index) answers, whose bits and face are unchanged;
    sd is negative where w > 0.5, NaN for a point with a non-finite coordinate and +inf when the mesh has no valid face.
    `index`: "bvh" (one hierarchy serves both queries) or "grid"."""
    index = check_distance_index(index)
    beta, lo, hi, _ = check_winding_args(mesh, lo, hi, beta, points=points)
    near = _index(mesh, lo, hi, None, index)
    dist2, face = near.query(points)
    w, _ = MeshWinding(mesh, lo, hi, bvh=near if index == "bvh" else None).query(points, beta)
    sd = dist2.double().sqrt().float()
    return torch.where(w > WINDING_INSIDE, -sd, sd), face, w
