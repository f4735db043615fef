"""The ray-casting stage: where a ray meets a mesh (include/nerf_hip.h "mesh ray casting").  The rays are the
[n, 11] rows nerf_ray_gen writes for the field (o, d, tmin, tmax, three columns that are not read), t is in units of d, and the
face test is watertight: no ray slips between two faces that share an edge.  It changes no mesh.

  * `pack_rays(origins, dirs, tmin, tmax)` makes such rows from points and directions.
  * `MeshRaycast(mesh, lo, hi, bvh)` casts against a `MeshBVH` (its own, or the caller's: no workspace of its own).
    `.cast(rays)` answers, per ray, the nearest hit `RayHits(t, face, bary, visits)`; `.occluded(rays)` only whether there is one;
    `.visible(points, eyes, eps)` whether the segment from each point to its eye is free.
  * `raycast_frame(mesh, c2w, K, H, W, near, far)` is `rasterize`'s frame by rays through the pixel centres, and
    `render_mesh_rays` is `render_mesh` on it (raster.py's `_render` with this visibility pass).
  * `check_raycast_args` is the one check of their arguments."""
import math
from typing import NamedTuple, Optional

import torch

from ... import _native as N
from ...rendering.ray import gen_rays
from ._base import CHUNK, Mesh, _check_mesh_tensors, _clamped, _mark, _query_in_order, check_mesh_args
from ._checks import is_number, need_int, need_tensor
from .distance import DISTANCE_MAX_SAMPLES, MeshBVH, _morton_codes
from .raster import RASTER_NEAR, RASTER_SMALL_MAX, MeshFrame, _render, check_raster_args
from .texture import Texture, _check_texture, sample_texture

RAY_STRIDE = 11                   # NERF_RAY_STRIDE
RAYCAST_SLACK = 2.0 ** -30        # the boxes are widened by this share of the largest |coordinate|
RAYCAST_SORTED_QUERY = False      # rays in their own order by default (pixel order is coherent; measured: DESIGN.md section 42)


class RayHits(NamedTuple):
    t: torch.Tensor                       # [n] float32: the parameter of the nearest hit in units of d, +inf for a miss
    face: torch.Tensor                    # [n] int32: the face hit, the lowest index on equal t; -1 for a miss
    bary: torch.Tensor                    # [n, 2] float32: (wb, wc) on that face, as sample_texture takes them; NaN for a miss
    visits: torch.Tensor                  # [n, 2] int32: (faces tested, boxes tested)


def check_raycast_args(mesh, lo, hi, rays=None, far=math.inf):
    """(lo [3], hi [3], far) as (float lists, float); ValueError for a box with lo >= hi or a non-finite corner, a mesh whose
    tensors are not contiguous verts float32 [V, 3], faces int32 [F, 3], normals float32 [V, 3] and colors None or float32 [V, 3]
    on one device with V, F <= 2^24, `rays` that are not None and not a contiguous float32 [n, 11] tensor of at most 2^30 rows on
    the mesh's device, or a far that is not a number > 0 (+inf is allowed, NaN is not)."""
    _, lo, hi, _ = check_mesh_args(2, lo, hi)
    _check_mesh_tensors("raycast", mesh)
    if rays is not None:
        need_tensor(rays, "raycast: rays", torch.float32, (None, RAY_STRIDE), mesh.verts.device, "[n, 11]")
        if rays.shape[0] > DISTANCE_MAX_SAMPLES:
            raise ValueError(f"raycast: at most 2^30 rays, got {rays.shape[0]}")
    if not is_number(far) or math.isnan(float(far)) or not float(far) > 0.0:
        raise ValueError(f"raycast far must be a number > 0 or +inf, got {far!r}")
    return lo, hi, float(far)


def pack_rays(origins: torch.Tensor, dirs: torch.Tensor, tmin=0.0, tmax=math.inf) -> torch.Tensor:
    """float32 [n, 11]: origins [n, 3] in columns 0-2, dirs [n, 3] (not normalised: t counts in units of d) in 3-5, tmin and tmax
    (numbers, or tensors [n]) in 6 and 7, zeros in 8-10.  ValueError unless origins and dirs are float32 [n, 3] on one device."""
    need_tensor(origins, "raycast: origins", torch.float32, (None, 3), shown="[n, 3]")
    need_tensor(dirs, "raycast: dirs", torch.float32, (origins.shape[0], 3), origins.device, "[n, 3]")
    rays = torch.zeros(origins.shape[0], RAY_STRIDE, dtype=torch.float32, device=origins.device)
    rays[:, 0:3], rays[:, 3:6] = origins, dirs
    rays[:, 6], rays[:, 7] = tmin, tmax
    return rays


def _ray_order(lo, hi):
    """rays -> the permutation that sorts them by the Morton code of their origin on the box, then by the octant of their
    direction: the `order` of _query_in_order.  Torch plumbing; no result depends on it."""
    def order(rays):
        d = torch.nan_to_num(rays[:, 3:6], nan=0.0)
        octant = (d[:, 0] < 0).long() | ((d[:, 1] < 0).long() << 1) | ((d[:, 2] < 0).long() << 2)
        return torch.sort(_morton_codes(rays[:, 0:3], lo, hi) * 8 + octant).indices
    return order


class MeshRaycast:
    """Rays against `mesh` on a face hierarchy: `bvh` (a MeshBVH of this very mesh) or a new MeshBVH(mesh, lo, hi).  The box only
    shapes the tree (and enters the slack); rays may start and end anywhere.  Nothing is built beyond the hierarchy, which is
    only read: one serves any number of casts.  The mesh's tensors must not change while it is in use.  mark: the MeshBVH's
    stages when it is built here."""

    def __init__(self, mesh: Mesh, lo, hi, bvh: Optional[MeshBVH] = None, mark=None):
        lo, hi, _ = check_raycast_args(mesh, lo, hi)
        if bvh is None:
            bvh = MeshBVH(mesh, lo, hi, mark)
        elif not isinstance(bvh, MeshBVH) or bvh.mesh.verts is not mesh.verts or bvh.mesh.faces is not mesh.faces:
            raise ValueError("raycast: bvh must be a MeshBVH of this mesh")
        self.mesh, self.lo, self.hi, self.bvh = mesh, lo, hi, bvh
        self.V, self.F, self.P = bvh.V, bvh.F, bvh.P

    def _run(self, rays, sort, outs, call, mark):
        check_raycast_args(self.mesh, self.lo, self.hi, rays)
        sort = RAYCAST_SORTED_QUERY if sort is None else bool(sort)
        n, m, b = rays.shape[0], self.mesh, self.bvh
        return _query_in_order(rays, _ray_order(self.lo, self.hi) if sort else None, outs, lambda r, *o: N.check(
            call(N.ptr(r), n, N.ptr(m.verts), self.V, N.ptr(m.faces), self.F, *b._box, N.ptr(b._ws), *(N.ptr(x) for x in o), N.stream())),
            mark)

    def cast(self, rays: torch.Tensor, sort: Optional[bool] = None, mark=None) -> RayHits:
        """RayHits of rays [n, 11]: the nearest accepted hit with tmin <= t <= tmax, the lowest face index on equal t, bit for
        bit the scan over every face; (+inf, -1, NaN, NaN) for a miss; (NaN, -1, NaN, NaN) and no visits for a ray whose o or d
        is not finite, whose d is 0, or whose tmin or tmax is NaN or tmin < 0 (nerf_raycast: no host read, any number of calls
        per hierarchy).  `sort`: cast in the order of the origins' Morton codes, then the directions' octants, and scatter the
        answers back, the same bits (None: RAYCAST_SORTED_QUERY).  mark: _mark's hook ("sort", "query", "scatter")."""
        n, dev = (rays.shape[0] if torch.is_tensor(rays) and rays.dim() == 2 else 0), self.mesh.verts.device
        outs = (torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                torch.empty(n, 2, dtype=torch.float32, device=dev), torch.empty(n, 2, dtype=torch.int32, device=dev))
        return RayHits(*self._run(rays, sort, outs, N.lib().nerf_raycast, mark))

    def occluded(self, rays: torch.Tensor, sort: Optional[bool] = None, mark=None) -> torch.Tensor:
        """bool [n]: whether cast(rays) would answer a face; the walk stops at the first accepted hit (nerf_raycast_any)."""
        n, dev = (rays.shape[0] if torch.is_tensor(rays) and rays.dim() == 2 else 0), self.mesh.verts.device
        hit, = self._run(rays, sort, (torch.empty(n, dtype=torch.uint8, device=dev),), N.lib().nerf_raycast_any, mark)
        return hit != 0

    def visible(self, points: torch.Tensor, eyes: torch.Tensor, eps: float, sort: Optional[bool] = None) -> torch.Tensor:
        """bool [n]: whether the segment from points[i] towards eyes[i] (both [n, 3]; eyes may be one point [3]), shortened by
        `eps` (a finite number >= 0, a length) at both ends, meets no face.  Torch packing around `occluded`: unit directions,
        tmin = eps, tmax = the distance minus eps; a segment no longer than 2 eps is free."""
        need_tensor(points, "raycast: points", torch.float32, (None, 3), self.mesh.verts.device, "[n, 3]")
        if not is_number(eps) or not math.isfinite(float(eps)) or float(eps) < 0.0:
            raise ValueError(f"raycast eps must be a finite number >= 0, got {eps!r}")
        if not torch.is_tensor(eyes) or eyes.dtype != torch.float32 or eyes.device != points.device or \
                tuple(eyes.shape) not in ((3,), tuple(points.shape)):
            raise ValueError("raycast: eyes must be a float32 [3] or [n, 3] tensor on the points' device")
        d = eyes.expand_as(points) - points
        length = d.double().pow(2).sum(1).sqrt().float()
        there = length > 0                                             # a point on its eye: tmax = -1 < tmin, free
        unit = torch.where(there[:, None], d / length[:, None], torch.ones_like(d))
        rays = pack_rays(points, unit.contiguous(), float(eps), torch.where(there, length - float(eps), -torch.ones_like(length)))
        return ~self.occluded(rays, sort)


def _mesh_bounds(mesh: Mesh):
    """(lo [3], hi [3]) about the finite vertices, each side padded so that lo < hi (one read of six floats to the host); the unit
    box for a mesh without one.  It only shapes the tree."""
    v = mesh.verts
    fin = v[torch.isfinite(v).all(1)] if v.shape[0] else v
    if fin.shape[0] == 0:
        return [-1.0] * 3, [1.0] * 3
    mm = torch.stack([fin.min(0).values, fin.max(0).values]).double().cpu().tolist()
    pad = max(1e-6, 1e-3 * max(h - l for l, h in zip(*mm)), 1e-6 * max(abs(x) for row in mm for x in row))
    return [l - pad for l in mm[0]], [h + pad for h in mm[1]]


def raycast_frame(mesh: Mesh, c2w, K, H: int, W: int, near: float = RASTER_NEAR, far: float = math.inf, chunk: int = CHUNK,
                  caster: Optional[MeshRaycast] = None, mark=None):
    """(face [H, W] int32, bary [H, W, 2], depth [H, W], acc [H, W] float32, visits [H, W, 2] int32) of `mesh` along the rays of
    gen_rays through every pixel centre, `chunk` pixels a cast in pixel order, tmin = near and tmax = far: the nearest face, the
    weights of its second and third corner, t, and 1 where a face is hit.  The rays' camera-frame z is -1, so t is the distance
    along the optical axis: depth = t where hit, else 0, acc 1 or 0 and bary 0 at a miss are rasterize's conventions, and the
    result shades through the same lookup and goes into TSDFVolume.integrate unchanged.  Unlike rasterize nothing is snapped and a
    face that crosses the near plane is cut there, not dropped.  `caster`: a MeshRaycast of this mesh to reuse (None: one is built
    on the box of the finite vertices).  No result depends on `chunk`.  mark: _mark's hook (the MeshBVH's stages, then "cast")."""
    _check_mesh_tensors("raycast_frame", mesh)
    H, W, near, _, _ = check_raster_args(H, W, near)
    chunk = need_int(chunk, "raycast chunk", 1, DISTANCE_MAX_SAMPLES)
    if caster is None:
        lo, hi = _mesh_bounds(mesh)
        caster = MeshRaycast(mesh, lo, hi, mark=mark)
    elif not isinstance(caster, MeshRaycast) or caster.mesh.verts is not mesh.verts or caster.mesh.faces is not mesh.faces:
        raise ValueError("raycast_frame: caster must be a MeshRaycast of this mesh")
    _, _, far = check_raycast_args(mesh, caster.lo, caster.hi, far=far)
    dev, n = mesh.verts.device, H * W
    t = torch.empty(n, dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    bary = torch.empty(n, 2, dtype=torch.float32, device=dev)
    visits = torch.empty(n, 2, dtype=torch.int32, device=dev)
    chunk = _clamped(chunk, n)
    _mark(mark, "cast")
    for p0 in range(0, n, chunk):
        cnt = min(chunk, n - p0)
        rays = gen_rays(H, W, K, c2w, near, far, torch.arange(p0, p0 + cnt, dtype=torch.int64, device=dev))
        hits = caster.cast(rays, sort=False)                           # pixel order is coherent already
        t[p0:p0 + cnt], face[p0:p0 + cnt], bary[p0:p0 + cnt], visits[p0:p0 + cnt] = hits
    hit = face >= 0
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    return (face.view(H, W), torch.where(hit[:, None], bary, zero).view(H, W, 2), torch.where(hit, t, zero).view(H, W),
            hit.float().view(H, W), visits.view(H, W, 2))


def render_mesh_rays(mesh: Mesh, c2w, K, H: int, W: int, texture: Optional[Texture] = None, background=None,
                     near: float = RASTER_NEAR, far: float = math.inf, caster: Optional[MeshRaycast] = None, mark=None) -> MeshFrame:
    """render_mesh with raycast_frame in place of rasterize: the same checks, lookup, background and nerf_raster_shade
    (raster.py's _render), on the face and barycentrics the rays find.  mark: raycast_frame's stages, then "texture" (with one)
    and "shade"."""
    def lookup(face, bary, near):
        _mark(mark, "texture")
        return sample_texture(texture, mesh, face, bary)

    def prepare():
        check_raycast_args(mesh, [0.0] * 3, [1.0] * 3, far=far)
        if texture is not None:
            _check_texture("render_mesh_rays", texture, mesh)
            return lookup
        if mesh.colors is None:
            raise ValueError("render_mesh_rays: a mesh without colors needs a texture")

    return _render("render_mesh_rays", mesh, c2w, K, H, W, prepare, background, near, False, mark, RASTER_SMALL_MAX,
                   visibility=lambda near_: raycast_frame(mesh, c2w, K, H, W, near_, far, caster=caster, mark=mark))
