"""The distance stage: how far one mesh is from another (include/nerf_hip.h "mesh distance").  It changes no
mesh.

  * `sample_surface(mesh, n, lo, hi, seed)` draws n points on the surface in proportion to area, counter-based: sample i of a seed
    is the same point whatever n is.
  * `MeshIndex(mesh, lo, hi, grid)` enters the faces into a `grid`^3 lattice of the box once; `.query(points)` answers, per point,
    the squared distance to the closest face and that face, bit for bit what a scan over every face answers (`grid=1` is that
    scan).  `point_mesh_distance` is the one-shot form.
  * `MeshBVH(mesh, lo, hi)` is the second index with the same answers, bit for bit: a bounding-volume hierarchy over the
    Morton-sorted faces (include/nerf_hip.h "mesh BVH"), whose cost does not grow with the empty space
    between a point and the surface.  `index="bvh"` selects it in `point_mesh_distance` and `mesh_distance`; "grid" is the default.
  * `closest_points(mesh, points, face)` is the closest point of the given face per point: the q behind the query's dist2.
  * `mesh_distance(a, b, n, lo, hi, seed, tau)` samples both meshes, queries each set against the other mesh and reduces: mean,
    RMS and Hausdorff distance per direction and symmetric, and with `tau` precision, recall and F-score.
  * `check_distance_args` is the one check of their arguments."""
import math
from typing import NamedTuple, Optional, Sequence

import torch

from ... import _native as N
from ._base import Mesh, _box, _check_mesh_tensors, _mark, _query_in_order, _rows, check_mesh_args
from ._checks import need_int, need_real, need_tensor

DISTANCE_MAX_GRID = 256
DISTANCE_MAX_SAMPLES = 1 << 30
DISTANCE_MAX_ENTRIES = 1 << 30
DISTANCE_INDEXES = ("grid", "bvh")
DISTANCE_SORTED_QUERY = True      # query in cell-sorted order (measured 2.4 - 3.2 times faster on 2^20 samples: DESIGN.md section 37)


def default_distance_grid(F: int) -> int:
    """The grid of MeshIndex(grid=None) for a mesh of F faces: isqrt(F // 32) clamped to [1, 256].  A surface of F faces meets
    about G^2 cells of a G^3 grid, so this aims at some tens of faces a cell; F stands in for the number of valid faces, which
    only a device pass knows and which it bounds."""
    return min(DISTANCE_MAX_GRID, max(1, math.isqrt(F // 32)))


def check_distance_args(mesh, n, lo: Sequence[float], hi: Sequence[float], grid=None, seed=0, tau=None, points=None):
    """(n, lo [3], hi [3], grid, seed, tau) as (int, float lists, int or None, int, float or None); ValueError for an n that is a
    bool, non-integral or outside [0, 2^30], a grid that is neither None nor such an int in [1, 256], a seed outside [0, 2^64),
    a tau that is neither None nor a finite number > 0, a box with lo >= hi or a non-finite corner, a mesh whose tensors are not
    contiguous verts float32 [V, 3], faces int32 [F, 3], normals float32 [V, 3] and colors None or float32 [V, 3] on one device
    with V, F <= 2^24, or `points` that are not None and not a contiguous float32 [n, 3] tensor on the mesh's device."""
    n = need_int(n, "distance n", 0, DISTANCE_MAX_SAMPLES)
    if grid is not None:
        grid = need_int(grid, "distance grid", 1, DISTANCE_MAX_GRID, want=f"None or an int in [1, {DISTANCE_MAX_GRID}]")
    seed = need_int(seed, "distance seed", 0, (1 << 64) - 1)
    if tau is not None:
        tau = need_real(tau, "distance tau", want="None or a finite number > 0", above=0.0)
    _, lo, hi, _ = check_mesh_args(2, lo, hi)
    _check_mesh_tensors("distance", mesh)
    if points is not None:
        need_tensor(points, "distance: points", torch.float32, (n, 3), mesh.verts.device, "[n, 3]")
    return n, lo, hi, grid, seed, tau


def sample_surface(mesh: Mesh, n: int, lo, hi, seed: int = 0, mark=None):
    """(points float32 [n, 3], face int32 [n]): n points on the mesh, a face drawn with probability proportional to its float32
    area (as an exact integer weight: the CDF does not depend on a summation order) and the point uniform on it.  Faces with an
    index out of range, a non-finite corner or no area are never drawn; the box [lo, hi] only fixes the unit of the weights.
    Sample i depends on (seed, i) alone (nerf_surface_cdf, one read of the total weight to the host, nerf_surface_sample).
    ValueError when n > 0 and the mesh has no area.  mark: _mark's hook ("cdf", "sample")."""
    n, lo, hi, _, seed, _ = check_distance_args(mesh, n, lo, hi, seed=seed)
    dev = mesh.verts.device
    V, F = mesh.verts.shape[0], mesh.faces.shape[0]
    points = torch.empty(n, 3, dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return points, face
    L = N.lib()
    clo, chi = _box(lo, hi)
    total = 0
    cdf = torch.empty(F, dtype=torch.int64, device=dev)
    if F:
        ws = torch.empty(L.nerf_surface_cdf_workspace_bytes(F), dtype=torch.uint8, device=dev)
        _mark(mark, "cdf")
        N.check(L.nerf_surface_cdf(N.ptr(mesh.verts), V, N.ptr(mesh.faces), F, clo, chi, N.ptr(ws), N.ptr(cdf), N.stream()))
        total = int(cdf[-1])                                  # the one host read
    _mark(mark, "sample")
    N.check(L.nerf_surface_sample(N.ptr(mesh.verts), V, N.ptr(mesh.faces), F, N.ptr(cdf), total, n, seed, N.ptr(points), N.ptr(face),
                                  N.stream()))
    return points, face


class MeshIndex:
    """The faces of `mesh` on a `grid`^3 lattice of the box [lo, hi] (grid=None: default_distance_grid(F); grid=1: one cell, the
    scan over every face): every valid face in every cell its bounding box, clamped onto the grid, overlaps (nerf_meshdist_count,
    one read of the entry count to the host, nerf_meshdist_build).  Faces may stick out of the box and points may lie outside it;
    the answers do not depend on the grid.  ValueError above 2^30 entries: use a coarser grid.  The index keeps the mesh's
    tensors; they must not change while it is in use.  mark: _mark's hook ("count", "build")."""

    def __init__(self, mesh: Mesh, lo, hi, grid=None, mark=None):
        _, lo, hi, grid, _, _ = check_distance_args(mesh, 0, lo, hi, grid=grid)
        self.mesh, self.lo, self.hi = mesh, lo, hi
        self.V, self.F = mesh.verts.shape[0], mesh.faces.shape[0]
        self.grid = default_distance_grid(self.F) if grid is None else grid
        dev = mesh.verts.device
        L = N.lib()
        self._box = _box(lo, hi)
        self._ws = torch.empty(L.nerf_meshdist_workspace_bytes(self.F, self.grid), dtype=torch.uint8, device=dev)
        tot = torch.empty(1, dtype=torch.int64, device=dev)
        _mark(mark, "count")
        N.check(L.nerf_meshdist_count(N.ptr(mesh.verts), self.V, N.ptr(mesh.faces), self.F, *self._box, self.grid, N.ptr(self._ws),
                                      N.ptr(tot), N.stream()))
        self.entries = int(tot[0])                            # the one host read
        if self.entries > DISTANCE_MAX_ENTRIES:
            raise ValueError(f"MeshIndex: {self.entries} entries at grid {self.grid} exceed 2^30; use a coarser grid")
        self._ent = torch.empty(self.entries, dtype=torch.int32, device=dev)
        _mark(mark, "build")
        N.check(L.nerf_meshdist_build(N.ptr(mesh.verts), self.V, N.ptr(mesh.faces), self.F, *self._box, self.grid, N.ptr(self._ws),
                                      N.ptr(self._ent), self.entries, N.stream()))

    def _cell_order(self, points):
        """The permutation that sorts the points by the linear index of their (clamped) cell: torch plumbing."""
        G = self.grid
        lo = torch.tensor(self.lo, dtype=torch.float64, device=points.device)
        ext = torch.tensor(self.hi, dtype=torch.float64, device=points.device) - lo
        c = ((torch.nan_to_num(points.double(), nan=0.0) - lo) * (G / ext)).floor().clamp_(0, G - 1).long()
        return torch.sort(c[:, 0] + G * (c[:, 1] + G * c[:, 2])).indices

    def query(self, points: torch.Tensor, sort: Optional[bool] = None, mark=None):
        """(dist2 float32 [n], face int32 [n]) of points [n, 3]: the squared distance to the closest valid face by Ericson's region
        tests in float32 and the lowest face index that attains it, bit for bit the scan over every face; NaN and -1 for a point
        with a non-finite coordinate, +inf and -1 when the mesh has no valid face (nerf_meshdist_query: no host read, any number
        of calls per index).  `sort`: query in cell-sorted order and scatter back, the same bits (None: DISTANCE_SORTED_QUERY).
        mark: _mark's hook ("sort", "query")."""
        n = _rows(points)
        check_distance_args(self.mesh, n, self.lo, self.hi, points=points)
        outs = (torch.empty(n, dtype=torch.float32, device=points.device), torch.empty(n, dtype=torch.int32, device=points.device))
        sort = DISTANCE_SORTED_QUERY if sort is None else bool(sort)
        return _query_in_order(points, self._cell_order if sort and self.grid > 1 else None, outs, lambda p, dist2, face: N.check(
            N.lib().nerf_meshdist_query(N.ptr(p), n, N.ptr(self.mesh.verts), self.V, N.ptr(self.mesh.faces), self.F, *self._box, self.grid,
                                        N.ptr(self._ws), N.ptr(self._ent), self.entries, N.ptr(dist2), N.ptr(face), N.stream())), mark)


BVH_SORTED_QUERY = True           # query in Morton order of the points (measured 1.4 - 1.9 times faster: DESIGN.md section 38)
BVH_LEAF = 4
BVH_CELLS = 4096


def _morton_codes(points, lo, hi):
    """int64 [n]: the 36-bit Morton code of each point's cell on the 4096^3 lattice of the box (clamped; NaN as 0), x lowest:
    torch plumbing, no result depends on it."""
    tlo = torch.tensor(lo, dtype=torch.float64, device=points.device)
    ext = torch.tensor(hi, dtype=torch.float64, device=points.device) - tlo
    c = ((torch.nan_to_num(points.double(), nan=0.0, posinf=0.0, neginf=0.0) - tlo) / ext * BVH_CELLS).floor().clamp_(0, BVH_CELLS - 1).long()
    c = (c | (c << 16)) & 0x00000000FF0000FF
    c = (c | (c << 8)) & 0x000000F00F00F00F
    c = (c | (c << 4)) & 0x00000030C30C30C3
    c = (c | (c << 2)) & 0x0000009249249249
    return c[:, 0] | (c[:, 1] << 1) | (c[:, 2] << 2)


def _morton_order(lo, hi):
    """points -> the permutation that sorts them by their Morton codes on the box: the `order` of _query_in_order."""
    return lambda points: torch.sort(_morton_codes(points, lo, hi)).indices


class MeshBVH:
    """The faces of `mesh` in a bounding-volume hierarchy: Morton keys of the faces' bounding-box midpoints on the 4096^3 lattice
    of the box [lo, hi] (nerf_bvh_keys), one torch.sort (the keys are unique), then leaves of four sorted faces under a complete
    binary tree of exact float32 boxes (nerf_bvh_build: no host read).  Faces may stick out of the box and points may lie outside
    it; the box only shapes the tree, never an answer.  The index keeps the mesh's tensors; they must not change while it is in
    use.  mark: _mark's hook ("keys", "sort_keys", "build")."""

    def __init__(self, mesh: Mesh, lo, hi, mark=None):
        _, lo, hi, _, _, _ = check_distance_args(mesh, 0, lo, hi)
        self.mesh, self.lo, self.hi = mesh, lo, hi
        self.V, self.F = mesh.verts.shape[0], mesh.faces.shape[0]
        self.leaves = -(-self.F // BVH_LEAF)
        self.P = 1 << max(self.leaves - 1, 0).bit_length()
        dev = mesh.verts.device
        L = N.lib()
        self._box = _box(lo, hi)
        self._ws = torch.empty(L.nerf_bvh_workspace_bytes(self.F), dtype=torch.uint8, device=dev)
        keys = torch.empty(self.F, dtype=torch.int64, device=dev)
        _mark(mark, "keys")
        N.check(L.nerf_bvh_keys(N.ptr(mesh.verts), self.V, N.ptr(mesh.faces), self.F, *self._box, N.ptr(keys), N.stream()))
        _mark(mark, "sort_keys")
        keys = torch.sort(keys).values
        _mark(mark, "build")
        N.check(L.nerf_bvh_build(N.ptr(mesh.verts), self.V, N.ptr(mesh.faces), self.F, N.ptr(keys), N.ptr(self._ws), N.stream()))

    @property
    def nodes(self):
        """float32 [2 P, 6]: node i as (min x y z, max x y z) in heap order; node 0 is unused.  A view: do not write."""
        return self._ws[:2 * self.P * 24].view(torch.float32).view(2 * self.P, 6)

    @property
    def order(self):
        """int32 [F]: the face of each sorted key, -1 for an invalid face.  A view: do not write."""
        at = (2 * self.P * 24 + 15) // 16 * 16
        return self._ws[at:at + 4 * self.F].view(torch.int32)

    def query(self, points: torch.Tensor, sort: Optional[bool] = None, mark=None):
        """(dist2 float32 [n], face int32 [n]) of points [n, 3]: MeshIndex.query's contract and its bits (nerf_bvh_query: no host
        read, any number of calls per index).  `sort`: query the points in the order of their own 36-bit Morton codes and scatter
        the answers back, the same bits (None: BVH_SORTED_QUERY).  mark: _mark's hook ("sort", "query", "scatter")."""
        n = _rows(points)
        check_distance_args(self.mesh, n, self.lo, self.hi, points=points)
        outs = (torch.empty(n, dtype=torch.float32, device=points.device), torch.empty(n, dtype=torch.int32, device=points.device))
        sort = BVH_SORTED_QUERY if sort is None else bool(sort)
        return _query_in_order(points, _morton_order(self.lo, self.hi) if sort else None, outs, lambda p, dist2, face: N.check(
            N.lib().nerf_bvh_query(N.ptr(p), n, N.ptr(self.mesh.verts), self.V, N.ptr(self.mesh.faces), self.F, *self._box, N.ptr(self._ws),
                                   N.ptr(dist2), N.ptr(face), N.stream())), mark)


def check_distance_index(index) -> str:
    """`index` as given; ValueError unless it is "grid" or "bvh"."""
    if not isinstance(index, str) or index not in DISTANCE_INDEXES:
        raise ValueError(f"distance index must be one of {DISTANCE_INDEXES}, got {index!r}")
    return index


def _index(mesh, lo, hi, grid, index):
    if index == "bvh":
        if grid is not None:
            raise ValueError(f"distance grid must be None with index='bvh', got {grid!r}")
        return MeshBVH(mesh, lo, hi)
    return MeshIndex(mesh, lo, hi, grid)


def point_mesh_distance(points: torch.Tensor, mesh: Mesh, lo, hi, grid=None, index="grid"):
    """MeshIndex(mesh, lo, hi, grid).query(points), or with index="bvh" MeshBVH(mesh, lo, hi).query(points): the same bits."""
    return _index(mesh, lo, hi, grid, check_distance_index(index)).query(points)


def closest_points(mesh: Mesh, points: torch.Tensor, face: torch.Tensor):
    """float32 [n, 3]: for points [n, 3] and face int32 [n] (a query's answer), the closest point of that face as the query
    computed it, so that dot(p - q, p - q) in float32 is the query's dist2 bit for bit; NaN for a face of -1, out of range or
    invalid (nerf_closest_points: one lane per point, no index needed)."""
    _check_mesh_tensors("distance", mesh)
    dev = mesh.verts.device
    n = _rows(points)
    need_tensor(points, "distance: points", torch.float32, (n, 3), dev, "[n, 3]")
    need_tensor(face, "distance: face", torch.int32, (n,), dev, "[n]")
    if n > DISTANCE_MAX_SAMPLES:
        raise ValueError(f"distance: at most 2^30 points, got {n}")
    out = torch.empty(n, 3, dtype=torch.float32, device=dev)
    if n:
        N.check(N.lib().nerf_closest_points(N.ptr(points), n, N.ptr(mesh.verts), mesh.verts.shape[0], N.ptr(mesh.faces),
                                            mesh.faces.shape[0], N.ptr(face), N.ptr(out), N.stream()))
    return out


class DistanceStats(NamedTuple):
    mean: float                           # of the distances (not squared)
    rms: float
    max: float                            # the one-sided Hausdorff distance of the samples


class MeshDistance(NamedTuple):
    a_to_b: DistanceStats                 # from the samples of a to the surface of b
    b_to_a: DistanceStats
    symmetric: DistanceStats              # over both sample sets; max is the Hausdorff distance
    precision: Optional[float]            # the share of a's samples within tau of b (None without tau)
    recall: Optional[float]               # the share of b's samples within tau of a
    fscore: Optional[float]               # their harmonic mean, 0 when both are 0
    points_a: torch.Tensor                # [n, 3] the samples of a
    points_b: torch.Tensor
    dist2_ab: torch.Tensor                # [n] float32 squared distance of points_a to b
    face_ab: torch.Tensor                 # [n] int32 the closest face of b
    dist2_ba: torch.Tensor
    face_ba: torch.Tensor


def _stats(d2: torch.Tensor) -> DistanceStats:
    d2 = d2.double()
    return DistanceStats(float(d2.sqrt().mean()), float(d2.mean().sqrt()), float(d2.max().sqrt()))


def mesh_distance(a: Mesh, b: Mesh, n: int, lo, hi, seed: int = 0, tau=None, grid=None, mark=None, index="grid") -> MeshDistance:
    """The distance between two meshes from n >= 1 area-weighted samples a side (the samples of `seed` on each): every sample of
    a is taken to the surface of b and the reverse; mean, RMS and largest distance per direction, and symmetric (the mean over
    both sets, the Hausdorff distance).  With `tau`, precision = the share of a's samples within tau of b, recall = the share of
    b's within tau of a, and their F-score, a being the reconstruction and b the truth.  Roots and reductions are torch float64 on
    the kernels' float32 squared distances, which the result carries.  `index`: "grid" (MeshIndex) or "bvh" (MeshBVH, the
    better choice when the meshes lie cells apart: DESIGN.md section 38); every field is the same.  mark: _mark's hook
    ("sample_a", "index_b", "query_ab", "sample_b", "index_a", "query_ba", "reduce")."""
    index = check_distance_index(index)
    n, lo, hi, grid, seed, tau = check_distance_args(a, n, lo, hi, grid=grid, seed=seed, tau=tau)
    check_distance_args(b, n, lo, hi)
    if n < 1:
        raise ValueError(f"distance n must be an int in [1, {DISTANCE_MAX_SAMPLES}] for mesh_distance, got {n!r}")
    _mark(mark, "sample_a")
    pa, _ = sample_surface(a, n, lo, hi, seed)
    _mark(mark, "index_b")
    ib = _index(b, lo, hi, grid, index)
    _mark(mark, "query_ab")
    d_ab, f_ab = ib.query(pa)
    _mark(mark, "sample_b")
    pb, _ = sample_surface(b, n, lo, hi, seed)
    _mark(mark, "index_a")
    ia = _index(a, lo, hi, grid, index)
    _mark(mark, "query_ba")
    d_ba, f_ba = ia.query(pb)
    _mark(mark, "reduce")
    s_ab, s_ba = _stats(d_ab), _stats(d_ba)
    sym = DistanceStats(0.5 * (s_ab.mean + s_ba.mean), math.sqrt(0.5 * (s_ab.rms ** 2 + s_ba.rms ** 2)), max(s_ab.max, s_ba.max))
    precision = recall = fscore = None
    if tau is not None:
        t2 = tau * tau
        precision = float((d_ab.double() <= t2).double().mean())
        recall = float((d_ba.double() <= t2).double().mean())
        fscore = 2.0 * precision * recall / (precision + recall) if precision + recall > 0.0 else 0.0
    return MeshDistance(s_ab, s_ba, sym, precision, recall, fscore, pa, pb, d_ab, f_ab, d_ba, f_ba)
