"""Mesh extraction from a trained field: marching cubes over its density volume (include/nerf_hip.h "mesh extraction", DESIGN.md
section 14).  The reference has no such export; this is Instant-NGP's.

  * `marching_cubes(volume, iso, lo, hi)` turns a float32 [R, R, R] device volume (vol[k, j, i] at the cell centres
    lo + (i + 0.5) h of the box) into a welded, consistently oriented triangle mesh: nerf_mesh_count, one read of (V, F) to the
    host, nerf_mesh_write_vertices, nerf_mesh_write_faces.
  * `Trainer.density_volume` / `Trainer.extract_mesh` (engine/trainer.py) sample the field on that lattice with its fused query
    (nerf_mesh_points, the query, nerf_occ_merge_ex with decay 0) and colour the vertices by a query along -normal.
  * `connected_components(volume, iso)` labels the 6-connected components of {v > iso}; `filter_components` sets the small ones
    (or all but the largest) to `iso`, which removes their pieces from the mesh and leaves the rest of it bit for bit
    (include/nerf_hip.h "connected components").  `extract(..., min_component, largest_only)` runs it
    between the density volume and marching cubes.
  * `erode(volume, iso, radius)` takes `radius` 6-neighbour layers off {v > iso} (the box faces erode too), which cuts the thin
    bridges that tie a floater to the surface; `reconstruct(volume, kept, iso, radius)` grows what was kept back inside
    {v > iso} by exactly `radius` geodesic steps; `open_components` is erode -> filter_components on the core -> reconstruct
    (include/nerf_hip.h "morphological opening").  `extract(..., opening_radius)` runs it in place of the
    plain filter; `min_component` then counts core voxels.
  * `TSDFVolume(resolution, lo, hi, trunc)` fuses rendered depth / opacity maps of posed cameras into a truncated signed distance
    volume on the same lattice (nerf_tsdf_integrate, 16 views per launch); `.volume()` is a volume for everything above at
    iso = 0 (include/nerf_hip.h "TSDF fusion").  `NGPTrainer.extract_mesh_tsdf` renders, fuses and meshes.
  * `simplify(mesh, grid, lo, hi, placement)` decimates a mesh by vertex clustering on a `grid`^3 lattice of the box, one vertex
    per occupied cell placed by the cell's quadric (box corners and edges survive) or at the mean; opposite faces that land on
    the same three cells annihilate, so one-voxel-thick sheets vanish (include/nerf_hip.h "mesh simplification", DESIGN.md
    section 27).  `extract(..., simplify_grid, simplify_placement)` runs it between marching cubes and the colour query.
  * `smooth(mesh, iterations, lo, hi, lam, mu)` moves the vertices by `iterations` pairs of Taubin's lambda|mu umbrella steps
    (mu = 0: plain Laplacian) and recomputes the normals from the faces; the faces and the colours are the input's
    (include/nerf_hip.h "mesh smoothing").  `extract(..., smooth_iterations, smooth_lambda, smooth_mu)`
    runs it between marching cubes and the simplifier.
  * `bake_texture(query, mesh, texels)` bakes a texture atlas for a finished mesh, one field query per texel: a right triangle
    of `texels` texels a leg per face, two faces to a cell, gutters extrapolated so that bilinear lookups do not bleed
    (include/nerf_hip.h "texture atlas"); `sample_texture` looks it up at surface samples.  A separate
    step behind `extract`: the pipeline's keywords are what they were.
  * `rasterize(mesh, c2w, K, H, W)` finds the face every pixel centre of a posed pinhole camera sees, its barycentrics and its
    depth, by exact integer coverage and one 64-bit atomicMin per covered pixel; `render_mesh` shades that with the vertex
    colours or through `sample_texture` into a `MeshFrame` (include/nerf_hip.h "mesh rendering"), so a
    mesh can be compared with the held-out frame and with the field's render in image space (`Trainer.mesh_psnr`).
  * `project_texture(mesh, images, c2w, K, texels, depth_tol)` colours the same atlas from posed pictures: every texel takes what
    the views saw of it where the mesh's own depth map of the view says it is visible, blended by the cosine or from the best
    view, and a fallback texture elsewhere (include/nerf_hip.h "view-projected texture").
  * `build_mipmaps(texture, mesh)` reduces an atlas face by face into a `TexturePyramid` of complete textures, `face_lod` gives
    every face a level of detail from its footprint on a camera's screen, and `sample_texture_mip` / `render_mesh_mip` look the
    pyramid up trilinearly, so a face that covers one pixel is not point-sampled from 45 texels (include/nerf_hip.h "texture mip
    pyramid").
  * `write_ply` writes a binary little-endian PLY; `write_obj` an OBJ with its .mtl and the atlas as a .png, which a PLY cannot
    carry.
"""
import ctypes as C
import math
import numbers
import os
import struct
import zlib
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from .. import _native as N

MAX_RES = 512                # NERF_MESH_MAX_RES
MAX_OPENING_RADIUS = 16      # NERF_MORPH_MAX_RADIUS
TSDF_MAX_VIEWS = 16          # NERF_TSDF_MAX_VIEWS
CHUNK = 1 << 19              # lattice points (or vertices) per query, as OccupancyGrid.update
RELU, EXP = 0, 1             # NERF_OCC_RELU / NERF_OCC_EXP
PLACEMENTS = {"mean": 0, "quadric": 1}   # NERF_SIMPLIFY_MEAN / NERF_SIMPLIFY_QUADRIC
SIMPLIFY_MAX_ITEMS = 1 << 24  # vertices, faces
SIMPLIFY_MAX_CLUSTERS = 1 << 21
SMOOTH_MAX_ITERATIONS = 1024
TEXTURE_MAX_TEXELS = 64      # texels per triangle leg
TEXTURE_MAX_SIDE = 16384     # NERF_TEXTURE_MAX_SIDE
RASTER_MAX_SIDE = 16384      # image height and width of the mesh renderer
RASTER_SMALL_MAX = 16        # NERF_RASTER_SMALL_MAX
RASTER_NEAR = 0.01           # the mesh renderer's default near plane
MIP_MAX_LEVELS = 6           # NERF_MIP_MAX_LEVELS: levels of a texture pyramid
PROJECT_MAX_VIEWS = 16       # NERF_PROJECT_MAX_VIEWS: views per launch of the projective bake
PROJECT_MODES = {"blend": 0, "best": 1}   # NERF_PROJECT_BLEND / NERF_PROJECT_BEST
PROJECT_COS_MIN = 0.05       # the projective bake's default grazing limit: the best of the sweep of DESIGN.md section 33
PROJECT_DEPTH_TOL_CELLS = 4.0  # Trainer.project_texture's default depth_tol in spacings of a 256^3 lattice on its scene box (section 33)


class Mesh(NamedTuple):
    verts: torch.Tensor                   # [V, 3] float32
    faces: torch.Tensor                   # [F, 3] int32, counter-clockwise seen from outside
    normals: torch.Tensor                 # [V, 3] float32, unit or 0
    colors: Optional[torch.Tensor] = None  # [V, 3] float32 in [0, 1], or None


def check_mesh_args(resolution, lo: Sequence[float], hi: Sequence[float], iso=0.0):
    """(R, lo [3], hi [3], iso) as (int, float lists, float); ValueError for R outside [2, MAX_RES], a box with lo >= hi or a
    non-finite corner, or a non-finite iso."""
    if isinstance(resolution, bool) or not isinstance(resolution, numbers.Integral) or not 2 <= int(resolution) <= MAX_RES:
        raise ValueError(f"mesh resolution must be an int in [2, {MAX_RES}], got {resolution!r}")
    lo = [float(x) for x in lo]
    hi = [float(x) for x in hi]
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError(f"mesh box: lo and hi need 3 coordinates each, got {lo!r}, {hi!r}")
    if not all(math.isfinite(a) and math.isfinite(b) and a < b for a, b in zip(lo, hi)):
        raise ValueError(f"mesh box: need finite lo < hi on every axis, got lo={lo!r}, hi={hi!r}")
    if isinstance(iso, bool) or not isinstance(iso, numbers.Real) or not math.isfinite(float(iso)):
        raise ValueError(f"mesh iso level must be a finite number, got {iso!r}")
    return int(resolution), lo, hi, float(iso)


def _box(lo, hi):
    return (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)


def lattice_rows(resolution: int, lo, hi, p0: int = 0, count: Optional[int] = None, device="cuda"):
    """(rays [count, 11], z [count, 1]) of lattice points [p0, p0 + count): o = the point, the rest 0 (nerf_mesh_points)."""
    R, lo, hi, _ = check_mesh_args(resolution, lo, hi)
    if count is None:
        count = R ** 3 - p0
    rays = torch.empty(count, 11, dtype=torch.float32, device=device)
    z = torch.empty(count, 1, dtype=torch.float32, device=device)
    _rows_into(R, lo, hi, p0, count, rays, z)
    return rays, z


def _rows_into(R, lo, hi, p0, count, rays, z):
    clo, chi = _box(lo, hi)
    N.check(N.lib().nerf_mesh_points(R, clo, chi, p0, count, N.ptr(rays) if count else None, N.ptr(z) if count else None,
                                     N.stream()))


def density_volume(query, activation: int, resolution: int, lo, hi, device="cuda", chunk: int = CHUNK) -> torch.Tensor:
    """float32 [R, R, R] = act(raw[..., 3]) of query(rays, z) -> raw [n, 1, 4] on the lattice, `chunk` points per query (the
    volume does not depend on it); act: RELU or EXP, NaN counting as 0."""
    R, lo, hi, _ = check_mesh_args(resolution, lo, hi)
    if activation not in (RELU, EXP):
        raise ValueError(f"density activation must be RELU (0) or EXP (1), got {activation!r}")
    n3 = R ** 3
    vol = torch.zeros(n3, dtype=torch.float32, device=device)
    chunk = max(1, min(int(chunk), n3))
    rays = torch.empty(chunk, 11, dtype=torch.float32, device=device)
    z = torch.empty(chunk, 1, dtype=torch.float32, device=device)
    for p0 in range(0, n3, chunk):
        cnt = min(chunk, n3 - p0)
        r, zz = rays[:cnt], z[:cnt]
        _rows_into(R, lo, hi, p0, cnt, r, zz)
        raw = N.f32(query(r, zz)).reshape(-1, 4)
        assert raw.shape[0] == cnt
        N.check(N.lib().nerf_occ_merge_ex(N.ptr(vol[p0:p0 + cnt]), N.ptr(raw), cnt, 0.0, activation, N.stream()))
    return vol.view(R, R, R)


def _check_volume(who, volume, iso, lo=(0.0,) * 3, hi=(1.0,) * 3):
    if not torch.is_tensor(volume) or volume.dim() != 3 or volume.dtype != torch.float32 or not volume.is_contiguous() \
            or not (volume.shape[0] == volume.shape[1] == volume.shape[2]):
        raise ValueError(f"{who}: volume must be a contiguous float32 [R, R, R] tensor")
    return check_mesh_args(volume.shape[0], lo, hi, iso)


def _mark(mark, stage):
    """The stage hook of connected_components, filter_components, erode, reconstruct, _open_components, _simplify and _smooth:
    mark(stage) just ahead of the stage's first C call (tools/ngp_mesh.py records a device event there).  None: nothing is
    called."""
    if mark is not None:
        mark(stage)


def _marching_cubes(volume, iso, lo, hi, color_rows: bool):
    R, lo, hi, iso = _check_volume("marching_cubes", volume, iso, lo, hi)
    dev = volume.device
    L = N.lib()
    clo, chi = _box(lo, hi)
    ws = torch.empty(L.nerf_mesh_workspace_bytes(R), dtype=torch.uint8, device=dev)
    tot = torch.empty(2, dtype=torch.int64, device=dev)
    N.check(L.nerf_mesh_count(N.ptr(volume), R, iso, N.ptr(ws), N.ptr(tot), N.stream()))
    V, F = tot.tolist()                                       # the one host read
    verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
    normals = torch.empty(V, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
    rows = torch.empty(V, 11, dtype=torch.float32, device=dev) if color_rows else None
    if V or F:
        N.check(L.nerf_mesh_write_vertices(N.ptr(volume), R, iso, clo, chi, N.ptr(ws), V, N.ptr(verts), N.ptr(normals),
                                           N.ptr(rows) if rows is not None else None, N.stream()))
        N.check(L.nerf_mesh_write_faces(N.ptr(volume), R, iso, N.ptr(ws), F, N.ptr(faces), N.stream()))
    return Mesh(verts, faces, normals), rows


def marching_cubes(volume: torch.Tensor, iso: float, lo, hi) -> Mesh:
    """The mesh of {v > iso} of a contiguous float32 [R, R, R] device volume on the lattice of the box [lo, hi] (no colours)."""
    return _marching_cubes(volume, iso, lo, hi, False)[0]


class Components(NamedTuple):
    labels: torch.Tensor                  # [R, R, R] int32: -1 outside, else the smallest linear index of the component
    sizes: torch.Tensor                   # [R, R, R] int32: the component's voxel count at its root, 0 elsewhere
    stats: torch.Tensor                   # [3] int64: components, inside voxels, the largest component's label or -1


def check_component_args(min_component, largest_only, resolution: int):
    """(min_component, largest_only) as (int, bool); ValueError for a min_component that is a bool, non-integral, negative or
    above R^3, or a largest_only that is not a bool."""
    if isinstance(min_component, bool) or not isinstance(min_component, numbers.Integral) \
            or not 0 <= int(min_component) <= int(resolution) ** 3:
        raise ValueError(f"min_component must be an int in [0, {int(resolution) ** 3}], got {min_component!r}")
    if not isinstance(largest_only, bool):
        raise ValueError(f"largest_only must be a bool, got {largest_only!r}")
    return int(min_component), largest_only


def connected_components(volume: torch.Tensor, iso: float, mark=None) -> Components:
    """The 6-connected components of {v > iso} of a contiguous float32 [R, R, R] device volume (include/nerf_hip.h "connected
    components"): nerf_ccl_label, nerf_ccl_sizes.  Device tensors; nothing is read on the host.  mark: _mark's hook ("label",
    "sizes")."""
    R, _, _, iso = _check_volume("connected_components", volume, iso)
    dev = volume.device
    L = N.lib()
    ws = torch.empty(L.nerf_ccl_workspace_bytes(R), dtype=torch.uint8, device=dev)
    labels = torch.empty(R, R, R, dtype=torch.int32, device=dev)
    sizes = torch.empty(R, R, R, dtype=torch.int32, device=dev)
    stats = torch.empty(3, dtype=torch.int64, device=dev)
    _mark(mark, "label")
    N.check(L.nerf_ccl_label(N.ptr(volume), R, iso, N.ptr(ws), N.ptr(labels), N.stream()))
    _mark(mark, "sizes")
    N.check(L.nerf_ccl_sizes(N.ptr(labels), R, N.ptr(sizes), N.ptr(stats), N.stream()))
    return Components(labels, sizes, stats)


def filter_components(volume: torch.Tensor, iso: float, min_component: int = 0, largest_only: bool = False,
                      components: Optional[Components] = None, mark=None) -> torch.Tensor:
    """A new volume in which every inside voxel of a component with fewer than `min_component` voxels -- and, with
    `largest_only`, of every component but the largest -- holds `iso` (outside); everything else is copied bit for bit
    (nerf_ccl_filter).  `components`: connected_components(volume, iso) when the caller has it already.  mark: _mark's hook
    ("label" and "sizes" when the components are computed here, then "filter")."""
    R, _, _, iso = _check_volume("filter_components", volume, iso)
    min_component, largest_only = check_component_args(min_component, largest_only, R)
    c = components if components is not None else connected_components(volume, iso, mark)
    for t, dt, shape in ((c.labels, torch.int32, (R, R, R)), (c.sizes, torch.int32, (R, R, R)), (c.stats, torch.int64, (3,))):
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != volume.device:
            raise ValueError("filter_components: components do not belong to this volume")
    out = torch.empty_like(volume)
    _mark(mark, "filter")
    N.check(N.lib().nerf_ccl_filter(N.ptr(volume), N.ptr(c.labels), N.ptr(c.sizes), N.ptr(c.stats), R, iso, min_component,
                                    int(largest_only), N.ptr(out), N.stream()))
    return out


def check_opening_args(opening_radius) -> int:
    """opening_radius as an int; ValueError for a bool, a non-integral value or one outside [0, MAX_OPENING_RADIUS] (0: no
    opening)."""
    if isinstance(opening_radius, bool) or not isinstance(opening_radius, numbers.Integral) \
            or not 0 <= int(opening_radius) <= MAX_OPENING_RADIUS:
        raise ValueError(f"opening_radius must be an int in [0, {MAX_OPENING_RADIUS}], got {opening_radius!r}")
    return int(opening_radius)


def _check_radius(who, radius) -> int:
    if check_opening_args(radius) < 1:
        raise ValueError(f"{who}: radius must be an int in [1, {MAX_OPENING_RADIUS}], got {radius!r}")
    return int(radius)


def erode(volume: torch.Tensor, iso: float, radius: int, mark=None):
    """(core, stats): `radius` steps of 6-neighbour erosion of {v > iso}, a neighbour beyond the lattice counting as outside;
    in the new volume `core` every inside voxel the erosion removed holds `iso`, everything else is copied bit for bit
    (nerf_morph_erode).  stats: int64 [2] device tensor = (inside voxels, core voxels); nothing is read on the host.
    mark: _mark's hook ("erode")."""
    R, _, _, iso = _check_volume("erode", volume, iso)
    radius = _check_radius("erode", radius)
    L = N.lib()
    ws = torch.empty(L.nerf_morph_workspace_bytes(R), dtype=torch.uint8, device=volume.device)
    core = torch.empty_like(volume)
    stats = torch.empty(2, dtype=torch.int64, device=volume.device)
    _mark(mark, "erode")
    N.check(L.nerf_morph_erode(N.ptr(volume), R, iso, radius, N.ptr(ws), N.ptr(core), N.ptr(stats), N.stream()))
    return core, stats


def reconstruct(volume: torch.Tensor, kept: torch.Tensor, iso: float, radius: int, mark=None):
    """(out, stats): the seeds {kept > iso} inside {volume > iso} grown by exactly `radius` 6-neighbour steps that never leave
    {volume > iso} (geodesic dilation); in the new volume `out` every inside voxel of `volume` they did not reach holds `iso`,
    everything else is copied bit for bit (nerf_morph_reconstruct).  `kept` must match `volume` in shape, dtype and device.
    stats: int64 [2] device tensor = (seed voxels, voxels reached); nothing is read on the host.
    mark: _mark's hook ("reconstruct")."""
    R, _, _, iso = _check_volume("reconstruct", volume, iso)
    radius = _check_radius("reconstruct", radius)
    if not torch.is_tensor(kept) or kept.shape != volume.shape or kept.dtype != volume.dtype or kept.device != volume.device \
            or not kept.is_contiguous():
        raise ValueError("reconstruct: kept must be a contiguous tensor of the volume's shape, dtype and device")
    L = N.lib()
    ws = torch.empty(L.nerf_morph_workspace_bytes(R), dtype=torch.uint8, device=volume.device)
    out = torch.empty_like(volume)
    stats = torch.empty(2, dtype=torch.int64, device=volume.device)
    _mark(mark, "reconstruct")
    N.check(L.nerf_morph_reconstruct(N.ptr(volume), N.ptr(kept), R, iso, radius, N.ptr(ws), N.ptr(out), N.ptr(stats), N.stream()))
    return out, stats


def open_components(volume: torch.Tensor, iso: float, radius: int, min_component: int = 0,
                    largest_only: bool = False) -> torch.Tensor:
    """A new volume: core = erode(volume, iso, radius); kept = filter_components(core, iso, min_component, largest_only) when
    min_component > 1 or largest_only, else the core itself (the plain opening by reconstruction); reconstruct(volume, kept, iso,
    radius).  `min_component` counts CORE voxels: a piece thinner than 2 radius + 1 voxels everywhere has none and is dropped
    whatever its size, and a field that thin everywhere yields an empty volume."""
    return _open_components(volume, iso, radius, min_component, largest_only)[0]


def _open_components(volume, iso, radius, min_component=0, largest_only=False, mark=None):
    """open_components with what it computes on the way: (opened volume, core, the core's Components or None when no filter ran,
    erode stats, reconstruct stats).  mark: _mark's hook ("erode", then "label", "sizes", "filter" when the filter runs,
    "reconstruct")."""
    R, _, _, iso = _check_volume("open_components", volume, iso)
    radius = _check_radius("open_components", radius)
    min_component, largest_only = check_component_args(min_component, largest_only, R)
    core, est = erode(volume, iso, radius, mark)
    kept, comps = core, None
    if min_component > 1 or largest_only:
        comps = connected_components(core, iso, mark)
        kept = filter_components(core, iso, min_component, largest_only, comps, mark)
    out, rst = reconstruct(volume, kept, iso, radius, mark)
    return out, core, comps, est, rst


def check_tsdf_args(trunc=None, acc_min=0.5, far=1.0, carve=True, min_views=1, H=1, W=1):
    """(trunc or None, acc_min, far, carve, min_views, H, W) as (float or None, float, float, bool, int, int, int); ValueError for
    a trunc or far that is not a finite number > 0 (trunc None: the volume's default), an acc_min outside (0, 1], a carve that is
    not a bool, a min_views that is not an int >= 1, or an H or W that is not an int in [1, 2^24]."""
    def real(x):
        return not isinstance(x, bool) and isinstance(x, numbers.Real) and math.isfinite(float(x))
    if trunc is not None and not (real(trunc) and float(trunc) > 0.0):
        raise ValueError(f"tsdf trunc must be None or a finite number > 0, got {trunc!r}")
    if not (real(acc_min) and 0.0 < float(acc_min) <= 1.0):
        raise ValueError(f"tsdf acc_min must be a number in (0, 1], got {acc_min!r}")
    if not (real(far) and float(far) > 0.0):
        raise ValueError(f"tsdf far must be a finite number > 0, got {far!r}")
    if not isinstance(carve, bool):
        raise ValueError(f"tsdf carve must be a bool, got {carve!r}")
    if isinstance(min_views, bool) or not isinstance(min_views, numbers.Integral) or int(min_views) < 1:
        raise ValueError(f"tsdf min_views must be an int >= 1, got {min_views!r}")
    for name, x in (("H", H), ("W", W)):
        if isinstance(x, bool) or not isinstance(x, numbers.Integral) or not 1 <= int(x) <= 1 << 24:
            raise ValueError(f"tsdf {name} must be an int in [1, 2^24], got {x!r}")
    return (None if trunc is None else float(trunc)), float(acc_min), float(far), carve, int(min_views), int(H), int(W)


def tsdf_views(c2w, K) -> np.ndarray:
    """float32 [n, 16]: per view c2w [3, 4] row-major, then fx, fy, cx, cy cast once from the K doubles (nerf_tsdf_view).
    c2w: [3, 4], [4, 4] or a stack of them; ValueError for another shape or a non-finite number."""
    c = np.asarray(c2w.detach().cpu().numpy() if torch.is_tensor(c2w) else c2w, np.float64)
    if c.ndim == 2:
        c = c[None]
    if c.ndim != 3 or c.shape[1] not in (3, 4) or c.shape[2] != 4:
        raise ValueError(f"tsdf c2w must be [3, 4], [4, 4] or a stack of them, got shape {tuple(c.shape)}")
    K = np.asarray(K.detach().cpu().numpy() if torch.is_tensor(K) else K, np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"tsdf K must be [3, 3], got shape {tuple(K.shape)}")
    v = np.empty((c.shape[0], 16), np.float32)
    v[:, :12] = c[:, :3, :].reshape(-1, 12)
    v[:, 12:] = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    if not np.isfinite(v).all():
        raise ValueError("tsdf: c2w and K must be finite")
    return v


class TSDFVolume:
    """A truncated signed distance volume on the mesh-extraction lattice of the box [lo, hi] at `resolution`, fused from depth
    / opacity maps (include/nerf_hip.h "TSDF fusion").  State: D (the running mean of the truncated distance in units of
    `trunc`), Wt (observations) float32 [R^3] and flags uint8 [R^3], zeroed.  trunc=None is 4 max_a(h_a), h_a = (hi_a - lo_a) / R
    in float32: wide enough that the mean over views whose depths disagree by a voxel or two still crosses zero between lattice
    points, and narrow enough that a wall 2 trunc thick keeps two sides (nerfstudio's default is a fixed world length; the
    lattice-relative choice keeps the band four voxels at every R)."""

    def __init__(self, resolution: int, lo, hi, trunc=None, device="cuda"):
        self.R, self.lo, self.hi, _ = check_mesh_args(resolution, lo, hi)
        trunc = check_tsdf_args(trunc=trunc)[0]
        if trunc is None:
            h = (np.asarray(self.hi, np.float32) - np.asarray(self.lo, np.float32)) / np.float32(self.R)
            trunc = float(np.float32(4.0) * h.max())
        self.trunc = float(np.float32(trunc))
        if not (math.isfinite(self.trunc) and self.trunc > 0.0):
            raise ValueError(f"tsdf trunc must be a positive float32, got {trunc!r}")
        self.device = torch.device(device)
        n3 = self.R ** 3
        self.D = torch.empty(n3, dtype=torch.float32, device=self.device)
        self.Wt = torch.empty(n3, dtype=torch.float32, device=self.device)
        self.flags = torch.empty(n3, dtype=torch.uint8, device=self.device)
        self.reset()

    def reset(self):
        """Zeroes D, Wt and flags (nerf_tsdf_reset)."""
        N.check(N.lib().nerf_tsdf_reset(N.ptr(self.D), N.ptr(self.Wt), N.ptr(self.flags), self.R, N.stream()))
        return self

    def integrate(self, depth, acc, c2w, K, H: int, W: int, acc_min: float = 0.5, far: float = 6.0, carve: bool = True):
        """Folds one view (depth, acc of H W elements, c2w [3, 4] or [4, 4]) or n stacked views ([n, ...]) into the state, in
        order, TSDF_MAX_VIEWS per launch (a longer stack is split here; the result does not depend on the split).  depth and
        acc are a renderer's aux maps (`render_rays(aux=True)`): depth = sum w z, not normalised.  A pixel with acc < acc_min
        says "nothing along this ray": with `carve` it is an observation of empty space for every voxel on the ray up to axial
        distance `far`, without it the pixel is ignored."""
        _, acc_min, far, carve, _, H, W = check_tsdf_args(None, acc_min, far, carve, 1, H, W)
        views = tsdf_views(c2w, K)
        n = views.shape[0]
        maps = []
        for name, t in (("depth", depth), ("acc", acc)):
            if not torch.is_tensor(t) or t.numel() != n * H * W:
                raise ValueError(f"tsdf {name} must be a tensor of {n} x {H} x {W} elements, got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
            maps.append(N.f32(t, self.device).reshape(n, H * W))
        clo, chi = _box(self.lo, self.hi)
        L = N.lib()
        for s in range(0, n, TSDF_MAX_VIEWS):
            m = min(TSDF_MAX_VIEWS, n - s)
            v = np.ascontiguousarray(views[s:s + m])
            N.check(L.nerf_tsdf_integrate(N.ptr(self.D), N.ptr(self.Wt), N.ptr(self.flags), self.R, clo, chi,
                                          v.ctypes.data_as(C.POINTER(C.c_float)), m, H, W, N.ptr(maps[0][s:s + m]),
                                          N.ptr(maps[1][s:s + m]), self.trunc, acc_min, far, int(carve), N.stream()))
        return self

    def volume(self, min_views: int = 1) -> torch.Tensor:
        """float32 [R, R, R] for marching_cubes / filter_components / open_components at iso = 0: -D where a voxel has at least
        `min_views` observations, +1 where it has fewer but was occluded in some view (seen only from behind a surface: inside),
        -1 otherwise (nerf_tsdf_volume)."""
        min_views = check_tsdf_args(min_views=min_views)[4]
        vol = torch.empty(self.R, self.R, self.R, dtype=torch.float32, device=self.device)
        N.check(N.lib().nerf_tsdf_volume(N.ptr(self.D), N.ptr(self.Wt), N.ptr(self.flags), self.R, min_views, N.ptr(vol),
                                         N.stream()))
        return vol


def vertex_colors(query, rows: torch.Tensor, chunk: int = CHUNK) -> torch.Tensor:
    """clamp(raw[..., :3], 0, 1) of query(rows, z = 0) -> raw [n, 1, 4] on the colour rows of nerf_mesh_write_vertices."""
    V = rows.shape[0]
    out = torch.empty(V, 3, dtype=torch.float32, device=rows.device)
    if V == 0:
        return out
    z = torch.zeros(min(V, chunk), 1, dtype=torch.float32, device=rows.device)
    for s in range(0, V, chunk):
        e = min(V, s + chunk)
        raw = query(rows[s:e], z[:e - s]).reshape(-1, 4)
        out[s:e] = raw[:, :3].clamp(0.0, 1.0)
    return out


def check_simplify_grid(grid) -> int:
    """simplify_grid as an int; ValueError for a bool, a non-integral value or one outside {0} + [2, MAX_RES] (0: no
    simplification)."""
    if isinstance(grid, bool) or not isinstance(grid, numbers.Integral) or not (int(grid) == 0 or 2 <= int(grid) <= MAX_RES):
        raise ValueError(f"simplify_grid must be 0 or an int in [2, {MAX_RES}], got {grid!r}")
    return int(grid)


def _check_mesh_tensors(who, mesh):
    """(V, F) of a Mesh whose tensors are contiguous verts float32 [V, 3], faces int32 [F, 3], normals float32 [V, 3] and colors
    None or float32 [V, 3] on one device, with V, F <= 2^24; ValueError otherwise (check_simplify_args, check_smooth_args,
    check_texture_args)."""
    if not isinstance(mesh, Mesh):
        raise ValueError(f"{who}: need an engine.mesh.Mesh, got {type(mesh).__name__}")

    def ok(t, dtype, rows=None):
        return torch.is_tensor(t) and t.dtype == dtype and t.dim() == 2 and t.shape[1] == 3 and t.is_contiguous() \
            and (rows is None or t.shape[0] == rows) and t.device == mesh.verts.device
    if not ok(mesh.verts, torch.float32):
        raise ValueError(f"{who}: verts must be a contiguous float32 [V, 3] tensor")
    V = mesh.verts.shape[0]
    if not ok(mesh.faces, torch.int32):
        raise ValueError(f"{who}: faces must be a contiguous int32 [F, 3] tensor on the vertices' device")
    if not ok(mesh.normals, torch.float32, V):
        raise ValueError(f"{who}: normals must be a contiguous float32 [V, 3] tensor on the vertices' device")
    if mesh.colors is not None and not ok(mesh.colors, torch.float32, V):
        raise ValueError(f"{who}: colors must be None or a contiguous float32 [V, 3] tensor on the vertices' device")
    F = mesh.faces.shape[0]
    if V > SIMPLIFY_MAX_ITEMS or F > SIMPLIFY_MAX_ITEMS:
        raise ValueError(f"{who}: at most 2^24 vertices and faces, got {V} and {F}")
    return V, F


def check_simplify_args(mesh, grid, lo: Sequence[float], hi: Sequence[float], placement="quadric"):
    """(grid, lo [3], hi [3], placement code) as (int, float lists, int); ValueError for a grid that is not an int in
    [2, MAX_RES], a placement other than "mean" / "quadric", a box with lo >= hi or a non-finite corner, or a mesh whose tensors
    are not contiguous verts float32 [V, 3], faces int32 [F, 3], normals float32 [V, 3] and colors None or float32 [V, 3] on one
    device, with V, F <= 2^24 and min(V, grid^3) <= 2^21."""
    if check_simplify_grid(grid) < 2:
        raise ValueError(f"simplify grid must be an int in [2, {MAX_RES}], got {grid!r}")
    grid, lo, hi, _ = check_mesh_args(int(grid), lo, hi)
    if not isinstance(placement, str) or placement not in PLACEMENTS:
        raise ValueError(f"simplify placement must be one of {sorted(PLACEMENTS)}, got {placement!r}")
    V, F = _check_mesh_tensors("simplify", mesh)
    if min(V, grid ** 3) > SIMPLIFY_MAX_CLUSTERS:
        raise ValueError(f"simplify: min(V, grid^3) = {min(V, grid ** 3)} possible clusters exceed 2^21; use a coarser grid")
    return grid, lo, hi, PLACEMENTS[placement]


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
    if isinstance(iterations, bool) or not isinstance(iterations, numbers.Integral) \
            or not 0 <= int(iterations) <= SMOOTH_MAX_ITERATIONS:
        raise ValueError(f"smooth iterations must be an int in [0, {SMOOTH_MAX_ITERATIONS}], got {iterations!r}")
    out = []
    for name, x in (("lambda", lam), ("mu", mu)):
        if isinstance(x, bool) or not isinstance(x, numbers.Real) or math.isnan(float(x)):
            raise ValueError(f"smooth {name} must be a number, got {x!r}")
        with np.errstate(over="ignore"):
            out.append(float(np.float32(float(x))))
    lam, mu = out
    if not 0.0 < lam <= 1.0:
        raise ValueError(f"smooth lambda must be in (0, 1] as a float32, got {lam!r}")
    if not (mu == 0.0 or -2.0 <= mu < 0.0):
        raise ValueError(f"smooth mu must be 0 (plain Laplacian) or in [-2, 0), got {mu!r}")
    return int(iterations), lam, mu


def check_smooth_args(mesh, iterations, lo: Sequence[float], hi: Sequence[float], lam=0.5, mu=-0.53):
    """(iterations, lo [3], hi [3], lam, mu) as (int, float lists, floats); ValueError for an iterations that is not an int in
    [1, SMOOTH_MAX_ITERATIONS], a lam outside (0, 1], a mu that is neither 0 nor in [-2, 0) (bools, non-numbers and NaN are
    refused), a box with lo >= hi or a non-finite corner, or a mesh whose tensors are not contiguous verts float32 [V, 3], faces
    int32 [F, 3], normals float32 [V, 3] and colors None or float32 [V, 3] on one device, with V, F <= 2^24."""
    iterations, lam, mu = check_smooth_params(iterations, lam, mu)
    if iterations < 1:
        raise ValueError(f"smooth iterations must be an int in [1, {SMOOTH_MAX_ITERATIONS}], got {iterations!r}")
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


def extract(query, activation: int, resolution: int, threshold: float, lo, hi, colors: bool = True, device="cuda",
            min_component: int = 0, largest_only: bool = False, opening_radius: int = 0, simplify_grid: int = 0,
            simplify_placement: str = "quadric", smooth_iterations: int = 0, smooth_lambda: float = 0.5,
            smooth_mu: float = -0.53) -> Mesh:
    """density_volume -> (with opening_radius > 0: open_components; else with min_component > 1 or largest_only:
    filter_components) -> marching_cubes at `threshold` -> (with smooth_iterations > 0: smooth) -> (with simplify_grid > 0:
    simplify on that grid of the box) -> (optionally) vertex colours, queried on the final mesh's rows: the field is asked once
    per vertex that is kept.  With opening_radius > 0 `min_component` counts core voxels (open_components).  With the defaults
    none of them is called."""
    check_mesh_args(resolution, lo, hi, threshold)
    min_component, largest_only = check_component_args(min_component, largest_only, resolution)
    opening_radius = check_opening_args(opening_radius)
    simplify_grid = check_simplify_grid(simplify_grid)
    if simplify_placement not in PLACEMENTS:
        raise ValueError(f"simplify placement must be one of {sorted(PLACEMENTS)}, got {simplify_placement!r}")
    check_smooth_params(smooth_iterations, smooth_lambda, smooth_mu)
    vol = density_volume(query, activation, resolution, lo, hi, device=device)
    if opening_radius > 0:
        vol = open_components(vol, threshold, opening_radius, min_component, largest_only)
    elif min_component > 1 or largest_only:
        vol = filter_components(vol, threshold, min_component, largest_only)
    return mesh_volume(query, vol, threshold, lo, hi, colors, simplify_grid, simplify_placement, smooth_iterations, smooth_lambda,
                       smooth_mu)


def mesh_volume(query, vol, iso, lo, hi, colors: bool, simplify_grid: int = 0, simplify_placement: str = "quadric",
                smooth_iterations: int = 0, smooth_lambda: float = 0.5, smooth_mu: float = -0.53) -> Mesh:
    """marching_cubes of `vol` at `iso` -> (with smooth_iterations > 0: smooth) -> (with simplify_grid > 0: simplify) -> (with
    `colors`) vertex_colors of `query` on the final mesh's rows [x, -n, 0, 0, -n]: the simplifier's, else the smoother's, else
    marching cubes'.  With smooth_iterations 0 and simplify_grid 0 the calls are those of marching cubes and the colour query
    alone."""
    smooth_iterations = check_smooth_params(smooth_iterations, smooth_lambda, smooth_mu)[0]
    if smooth_iterations > 0 or simplify_grid > 0:
        mesh, rows = _marching_cubes(vol, iso, lo, hi, False)[0], None
        if smooth_iterations > 0:
            mesh, rows = _smooth(mesh, smooth_iterations, lo, hi, smooth_lambda, smooth_mu, colors and simplify_grid == 0)
        if simplify_grid > 0:
            mesh, rows = _simplify(mesh, simplify_grid, lo, hi, simplify_placement, colors)[:2]
    else:
        mesh, rows = _marching_cubes(vol, iso, lo, hi, colors)
    if not colors:
        return mesh
    return mesh._replace(colors=vertex_colors(query, rows))


def write_ply(path: str, mesh: Mesh) -> str:
    """Binary little-endian PLY: vertex x y z nx ny nz (float) [+ red green blue (uchar, round(255 c))], face
    `list uchar int vertex_indices`.  Written under a temporary name, then renamed."""
    v = mesh.verts.detach().cpu().numpy().astype("<f4")
    n = mesh.normals.detach().cpu().numpy().astype("<f4")
    f = mesh.faces.detach().cpu().numpy().astype("<i4")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if mesh.colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vert = np.empty(len(v), dtype=fields)
    for k, name in enumerate("xyz"):
        vert[name] = v[:, k]
        vert["n" + name] = n[:, k]
    if mesh.colors is not None:
        c = np.clip(np.nan_to_num(mesh.colors.detach().cpu().numpy().astype(np.float64)), 0.0, 1.0)
        rgb = np.round(255.0 * c).astype(np.uint8)
        for k, name in enumerate(("red", "green", "blue")):
            vert[name] = rgb[:, k]
    face = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    face["n"] = 3
    face["i"] = f
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    head += [f"property {'float' if t == '<f4' else 'uchar'} {name}" for name, t in fields]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    tmp = path + ".tmp"
    with open(tmp, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())
    os.replace(tmp, path)
    return path


def read_ply(path: str) -> Mesh:
    """The inverse of write_ply (CPU tensors); only the layout write_ply produces."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    if head[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError(f"{path}: not a binary little-endian PLY")
    nv = int(head[2].split()[2])
    props = [ln.split() for ln in head if ln.startswith("property ") and "list" not in ln]
    fields = [(p[2], "<f4" if p[1] == "float" else "u1") for p in props]
    nf = int(next(ln for ln in head if ln.startswith("element face")).split()[2])
    vert = np.frombuffer(data, dtype=fields, count=nv, offset=end)
    face = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nf, offset=end + vert.nbytes)
    if end + vert.nbytes + face.nbytes != len(data) or not (face["n"] == 3).all():
        raise ValueError(f"{path}: unexpected PLY layout")
    verts = torch.from_numpy(np.stack([vert[k] for k in "xyz"], 1).copy())
    normals = torch.from_numpy(np.stack([vert["n" + k] for k in "xyz"], 1).copy())
    colors = None
    if "red" in vert.dtype.names:
        colors = torch.from_numpy(np.stack([vert[k] for k in ("red", "green", "blue")], 1).astype(np.float32) / 255.0)
    return Mesh(verts, torch.from_numpy(face["i"].copy()), normals, colors)


class Texture(NamedTuple):
    image: torch.Tensor                   # [H, W, 3] uint8, row 0 on top
    uv: torch.Tensor                      # [F, 3, 2] float32, (u, v) per corner, v upwards
    texels: int                           # T: texels per triangle leg


def texture_layout(F: int, texels: int):
    """(W, H, C, S) of the atlas of F faces at `texels` texels per triangle leg (nerf_texture_layout; no device needed):
    S = texels + 2 the cell side, C cells per row.  ValueError for F outside [0, 2^24], texels outside [2, TEXTURE_MAX_TEXELS] or
    an atlas side above TEXTURE_MAX_SIDE (the text names the largest texels that fits)."""
    out = (C.c_int64 * 4)()
    N.check(N.lib().nerf_texture_layout(int(F), int(texels), out))
    return tuple(int(x) for x in out)


def check_texture_args(mesh, texels=8):
    """(texels, (W, H, C, S)) as (int, ints); ValueError for a texels that is a bool, non-integral or outside
    [2, TEXTURE_MAX_TEXELS], an atlas wider or higher than TEXTURE_MAX_SIDE, or a mesh that check_smooth_args would refuse."""
    if isinstance(texels, bool) or not isinstance(texels, numbers.Integral) or not 2 <= int(texels) <= TEXTURE_MAX_TEXELS:
        raise ValueError(f"texture texels must be an int in [2, {TEXTURE_MAX_TEXELS}], got {texels!r}")
    _, F = _check_mesh_tensors("texture", mesh)
    return int(texels), texture_layout(F, int(texels))


def bake_texture(query, mesh: Mesh, texels: int = 8, chunk: int = CHUNK, mark=None) -> Texture:
    """The texture atlas of `mesh` (include/nerf_hip.h "texture atlas"): every face gets a right triangle
    of `texels` texels a leg, two faces to a square cell, and every texel the colour clamp(raw[..., :3], 0, 1) of
    query(rows, z = 0) -> raw [n, 1, 4] at its point of the face looking along minus the interpolated normal, as the vertex
    colour query does at the vertices.  `chunk` texels per query (nerf_texture_rows, the query, nerf_texture_store; the image
    does not depend on it), then nerf_texture_uv once; no host read.  F = 0: a black cell, no query.  The mesh is not changed.
    mark: _mark's hook ("rows", "query", "store" per chunk, then "uv")."""
    T, (W, H, _, _) = check_texture_args(mesh, texels)
    dev, V, F = mesh.verts.device, mesh.verts.shape[0], mesh.faces.shape[0]
    uv = torch.empty(F, 3, 2, dtype=torch.float32, device=dev)
    if F == 0:
        return Texture(torch.zeros(H, W, 3, dtype=torch.uint8, device=dev), uv, T)
    L = N.lib()
    image = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    P = W * H
    chunk = max(1, min(int(chunk), P))
    rows = torch.empty(chunk, 11, dtype=torch.float32, device=dev)
    z = torch.zeros(chunk, 1, dtype=torch.float32, device=dev)
    for p0 in range(0, P, chunk):
        cnt = min(chunk, P - p0)
        r = rows[:cnt]
        _mark(mark, "rows")
        N.check(L.nerf_texture_rows(N.ptr(mesh.verts), N.ptr(mesh.normals), V, N.ptr(mesh.faces), F, T, p0, cnt, N.ptr(r), N.stream()))
        _mark(mark, "query")
        raw = N.f32(query(r, z[:cnt]))
        if raw.numel() != 4 * cnt:
            raise ValueError(f"bake_texture: the query must return raw [{cnt}, 1, 4], got shape {tuple(raw.shape)}")
        raw = raw.reshape(-1, 4)
        if raw.data_ptr() % 16:
            raw = raw.clone()
        _mark(mark, "store")
        N.check(L.nerf_texture_store(N.ptr(raw), V, N.ptr(mesh.faces), F, T, p0, cnt, N.ptr(image), N.stream()))
    _mark(mark, "uv")
    N.check(L.nerf_texture_uv(F, T, N.ptr(uv), N.stream()))
    return Texture(image, uv, T)


def _check_texture(who, texture, mesh):
    """(texels, layout) of a Texture that belongs to `mesh`: an image of the layout's size and one uv triple per face, on the
    mesh's device."""
    if not isinstance(texture, Texture):
        raise ValueError(f"{who}: need an engine.mesh.Texture, got {type(texture).__name__}")
    T, lay = check_texture_args(mesh, texture.texels)
    F, dev = mesh.faces.shape[0], mesh.verts.device
    im, uv = texture.image, texture.uv
    if not torch.is_tensor(im) or im.dtype != torch.uint8 or tuple(im.shape) != (lay[1], lay[0], 3) or not im.is_contiguous() \
            or im.device != dev:
        raise ValueError(f"{who}: image must be a contiguous uint8 [{lay[1]}, {lay[0]}, 3] tensor on the vertices' device")
    if not torch.is_tensor(uv) or uv.dtype != torch.float32 or tuple(uv.shape) != (F, 3, 2) or not uv.is_contiguous() \
            or uv.device != dev:
        raise ValueError(f"{who}: uv must be a contiguous float32 [{F}, 3, 2] tensor on the vertices' device")
    return T, lay


def sample_texture(texture: Texture, mesh: Mesh, face: torch.Tensor, bary: torch.Tensor, rows: bool = False):
    """rgb float32 [n, 3]: the bilinear lookup of the atlas at the surface samples (face [n] int32, bary [n, 2] float32 =
    the weights (wb, wc) of the face's second and third corner, clamped into the triangle); a face outside [0, F) reads black.
    With `rows` also the query rows [n, 11] of the very points, as bake_texture asks them (nerf_texture_sample)."""
    T, _ = _check_texture("sample_texture", texture, mesh)
    dev = mesh.verts.device
    if not torch.is_tensor(face) or face.dtype != torch.int32 or face.dim() != 1 or not face.is_contiguous() or face.device != dev:
        raise ValueError("sample_texture: face must be a contiguous int32 [n] tensor on the vertices' device")
    n = face.shape[0]
    if not torch.is_tensor(bary) or bary.dtype != torch.float32 or tuple(bary.shape) != (n, 2) or not bary.is_contiguous() \
            or bary.device != dev:
        raise ValueError(f"sample_texture: bary must be a contiguous float32 [{n}, 2] tensor on the vertices' device")
    rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
    out = torch.empty(n, 11, dtype=torch.float32, device=dev) if rows else None
    if n:
        N.check(N.lib().nerf_texture_sample(N.ptr(texture.image), N.ptr(mesh.verts), N.ptr(mesh.normals), mesh.verts.shape[0],
                                            N.ptr(mesh.faces), mesh.faces.shape[0], T, N.ptr(face), N.ptr(bary), n, N.ptr(rgb),
                                            N.ptr(out), N.stream()))
    return (rgb, out) if rows else rgb


class MeshFrame(NamedTuple):
    rgb: torch.Tensor                     # [H, W, 3] float32
    depth: torch.Tensor                   # [H, W] float32: distance along the optical axis, 0 where empty
    acc: torch.Tensor                     # [H, W] float32: 1 where a face is seen, else 0
    face: torch.Tensor                    # [H, W] int32: the face seen, -1 where empty
    bary: torch.Tensor                    # [H, W, 2] float32: (wb, wc) on that face, as sample_texture takes them


def check_raster_args(H=1, W=1, near=RASTER_NEAR, cull_backfaces=False, small_max=RASTER_SMALL_MAX):
    """(H, W, near, cull_backfaces, small_max) as (int, int, float, bool, int); ValueError for an H or W that is not an int in
    [1, RASTER_MAX_SIDE], a near that is not a finite number > 0 (as a float32), a cull_backfaces that is not a bool or a
    small_max that is not an int in [0, 2^30]."""
    for name, x in (("H", H), ("W", W)):
        if isinstance(x, bool) or not isinstance(x, numbers.Integral) or not 1 <= int(x) <= RASTER_MAX_SIDE:
            raise ValueError(f"raster {name} must be an int in [1, {RASTER_MAX_SIDE}], got {x!r}")
    if isinstance(near, bool) or not isinstance(near, numbers.Real) or not math.isfinite(float(near)) \
            or not 0.0 < float(np.float32(near)) < math.inf:
        raise ValueError(f"raster near must be a finite number > 0, got {near!r}")
    if not isinstance(cull_backfaces, bool):
        raise ValueError(f"raster cull_backfaces must be a bool, got {cull_backfaces!r}")
    if isinstance(small_max, bool) or not isinstance(small_max, numbers.Integral) or not 0 <= int(small_max) <= 1 << 30:
        raise ValueError(f"raster small_max must be an int in [0, 2^30], got {small_max!r}")
    return int(H), int(W), float(near), cull_backfaces, int(small_max)


def _raster_view(c2w, K):
    views = tsdf_views(c2w, K)
    if views.shape[0] != 1:
        raise ValueError(f"raster: need one camera, got a stack of {views.shape[0]}")
    return np.ascontiguousarray(views[0]).ctypes.data_as(C.POINTER(C.c_float)), views


def rasterize(mesh: Mesh, c2w, K, H: int, W: int, near: float = RASTER_NEAR, cull_backfaces: bool = False, mark=None,
              small_max: int = RASTER_SMALL_MAX):
    """(face [H, W] int32, bary [H, W, 2], depth [H, W], acc [H, W] float32, stats [4] int64) of `mesh` seen by the pinhole
    camera (c2w [3, 4] or [4, 4], K [3, 3], as tsdf_views takes them) whose pixel centres are the rays of gen_rays
    (include/nerf_hip.h "mesh rendering"): the nearest face at every pixel centre, the weights of its
    second and third corner there, the distance along the optical axis, and 1 where a face is seen.  depth and acc go into
    TSDFVolume.integrate unchanged.  Faces with a vertex in front of `near` are dropped, not clipped.  stats (on the device):
    faces drawn, dropped for depth or guard band, dropped otherwise, key updates.  small_max: the largest bounding box, in
    pixels, that one lane walks; the result does not depend on it.  nerf_raster_clear, _draw, _resolve; no host read.  F = 0:
    nothing is launched.  mark: _mark's hook ("clear", "draw", "resolve")."""
    _check_mesh_tensors("rasterize", mesh)
    H, W, near, cull, small_max = check_raster_args(H, W, near, cull_backfaces, small_max)
    view, _keep = _raster_view(c2w, K)
    dev, V, F = mesh.verts.device, mesh.verts.shape[0], mesh.faces.shape[0]
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    if F == 0:
        return (torch.full((H, W), -1, dtype=torch.int32, device=dev), torch.zeros(H, W, 2, dtype=torch.float32, device=dev),
                torch.zeros(H, W, dtype=torch.float32, device=dev), torch.zeros(H, W, dtype=torch.float32, device=dev), stats)
    L = N.lib()
    keys = torch.empty(H * W, dtype=torch.int64, device=dev)
    face = torch.empty(H, W, dtype=torch.int32, device=dev)
    bary = torch.empty(H, W, 2, dtype=torch.float32, device=dev)
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    acc = torch.empty(H, W, dtype=torch.float32, device=dev)
    _mark(mark, "clear")
    N.check(L.nerf_raster_clear(N.ptr(keys), H, W, N.ptr(stats), N.stream()))
    _mark(mark, "draw")
    N.check(L.nerf_raster_draw(N.ptr(mesh.verts), V, N.ptr(mesh.faces), F, 0, view, H, W, near, int(cull), small_max, N.ptr(keys),
                               N.ptr(stats), N.stream()))
    _mark(mark, "resolve")
    N.check(L.nerf_raster_resolve(N.ptr(keys), N.ptr(mesh.verts), V, N.ptr(mesh.faces), F, view, H, W, near, N.ptr(face), N.ptr(bary),
                                  N.ptr(depth), N.ptr(acc), N.stream()))
    return face, bary, depth, acc, stats


def _raster_background(background, H, W, dev):
    """(tensor, per_pixel): None is white; one colour [3]; or one per pixel, [H W, 3] or [H, W, 3], as render_frame takes it."""
    if background is None:
        return torch.ones(3, dtype=torch.float32, device=dev), 0
    bg = N.f32(background, dev)
    if bg.numel() == 3:
        return bg.reshape(3), 0
    if bg.numel() == 3 * H * W and bg.shape[-1] == 3:
        return bg.reshape(H * W, 3), 1
    raise ValueError(f"render_mesh: background must be None, one colour [3] or [{H * W}, 3], got shape {tuple(bg.shape)}")


def render_mesh(mesh: Mesh, c2w, K, H: int, W: int, texture: Optional[Texture] = None, background=None, near: float = RASTER_NEAR,
                cull_backfaces: bool = False, mark=None, small_max: int = RASTER_SMALL_MAX) -> MeshFrame:
    """The picture of `mesh` from the camera of `rasterize`: with `texture` every covered pixel looks the atlas up at its
    (face, bary) through sample_texture; without one it takes the barycentric sum of mesh.colors (ValueError if there are none).
    Empty pixels take `background`: None is white, else one colour or one per pixel as Trainer.render_frame.  One sample at the
    pixel centre; no antialiasing.  mark: rasterize's stages, then "texture" (with one) and "shade"."""
    _check_mesh_tensors("render_mesh", mesh)
    H, W, near, cull_backfaces, small_max = check_raster_args(H, W, near, cull_backfaces, small_max)
    if texture is not None:
        _check_texture("render_mesh", texture, mesh)
    elif mesh.colors is None:
        raise ValueError("render_mesh: a mesh without colors needs a texture")
    dev, V, F = mesh.verts.device, mesh.verts.shape[0], mesh.faces.shape[0]
    bg, per_pixel = _raster_background(background, H, W, dev)
    face, bary, depth, acc, _ = rasterize(mesh, c2w, K, H, W, near, cull_backfaces, mark, small_max)
    if F == 0:
        rgb = (bg.reshape(H, W, 3) if per_pixel else bg.expand(H, W, 3)).clone()
        return MeshFrame(rgb, depth, acc, face, bary)
    looked_up = None
    if texture is not None:
        _mark(mark, "texture")
        looked_up = sample_texture(texture, mesh, face.reshape(-1), bary.reshape(-1, 2))
    rgb = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    _mark(mark, "shade")
    N.check(N.lib().nerf_raster_shade(N.ptr(face), N.ptr(bary), N.ptr(mesh.faces), V, F, None if texture is not None else N.ptr(mesh.colors),
                                      N.ptr(looked_up), N.ptr(bg), per_pixel, H, W, N.ptr(rgb), N.stream()))
    return MeshFrame(rgb, depth, acc, face, bary)


class TexturePyramid(NamedTuple):
    levels: tuple                         # of Texture: levels[0] the atlas itself, levels[l] at mip_levels(texels)[l] texels a leg


def mip_levels(texels: int) -> tuple:
    """(T_0, ..., T_{L-1}): the texels per triangle leg of the levels of a pyramid over an atlas of `texels` (nerf_mip_levels; no
    device needed): T_{l+1} = (T_l + 1) // 2 while T_l > 2, at most MIP_MAX_LEVELS.  ValueError for texels outside
    [2, TEXTURE_MAX_TEXELS]."""
    if isinstance(texels, bool) or not isinstance(texels, numbers.Integral):
        raise ValueError(f"mip texels must be an int in [2, {TEXTURE_MAX_TEXELS}], got {texels!r}")
    out = (C.c_int32 * (1 + MIP_MAX_LEVELS))()
    N.check(N.lib().nerf_mip_levels(int(texels), out))
    return tuple(int(x) for x in out[1:1 + out[0]])


def build_mipmaps(texture: Texture, mesh: Mesh, chunk: int = CHUNK, mark=None) -> TexturePyramid:
    """The mip pyramid of `texture` (bake_texture's or project_texture's) of `mesh` (include/nerf_hip.h "texture mip pyramid",
    DESIGN.md section 34): level l + 1 is reduced from level l face by face, nine bilinear taps inside the face's own triangle per
    texel and gutters extrapolated from the coarse bytes, so every level is a complete Texture that sample_texture, render_mesh
    and write_obj take unchanged.  levels[0] is `texture` itself.  `chunk` coarse texels per launch of nerf_mip_reduce (the images
    do not depend on it), then nerf_texture_uv once per level; no host read.  F = 0: black cells, nothing is launched.  mark:
    _mark's hook ("reduce" and "uv" once per level, in that order)."""
    T, _ = _check_texture("build_mipmaps", texture, mesh)
    dev, F = mesh.verts.device, mesh.faces.shape[0]
    L = N.lib()
    levels = [texture]
    for Tl in mip_levels(T)[1:]:
        W, H, _, _ = texture_layout(F, Tl)
        uv = torch.empty(F, 3, 2, dtype=torch.float32, device=dev)
        if F == 0:
            levels.append(Texture(torch.zeros(H, W, 3, dtype=torch.uint8, device=dev), uv, Tl))
            continue
        fine = levels[-1]
        image = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
        P = W * H
        step = max(1, min(int(chunk), P))
        _mark(mark, "reduce")
        for p0 in range(0, P, step):
            N.check(L.nerf_mip_reduce(N.ptr(fine.image), F, fine.texels, N.ptr(image), p0, min(step, P - p0), N.stream()))
        _mark(mark, "uv")
        N.check(L.nerf_texture_uv(F, Tl, N.ptr(uv), N.stream()))
        levels.append(Texture(image, uv, Tl))
    return TexturePyramid(tuple(levels))


def _check_pyramid(who, pyramid, mesh):
    """The texels of level 0 of a TexturePyramid that belongs to `mesh`: every level a Texture of the mesh (_check_texture) and
    their texels the chain mip_levels(levels[0].texels)."""
    if not isinstance(pyramid, TexturePyramid) or not isinstance(pyramid.levels, tuple) or not pyramid.levels:
        raise ValueError(f"{who}: need an engine.mesh.TexturePyramid with at least one level, got {type(pyramid).__name__}")
    for level in pyramid.levels:
        _check_texture(who, level, mesh)
    chain = mip_levels(pyramid.levels[0].texels)
    if tuple(level.texels for level in pyramid.levels) != chain:
        raise ValueError(f"{who}: the levels must have {chain} texels a leg, got {tuple(level.texels for level in pyramid.levels)}")
    return chain[0]


def check_lod_scale(scale) -> float:
    """`scale` as a float; ValueError unless it is a finite number > 0 (as a float32)."""
    ok = not isinstance(scale, bool) and isinstance(scale, numbers.Real) and math.isfinite(float(scale))
    if ok:
        with np.errstate(over="ignore"):
            ok = 0.0 < float(np.float32(scale)) < math.inf
    if not ok:
        raise ValueError(f"mip lod scale must be a finite number > 0, got {scale!r}")
    return float(scale)


def face_lod(mesh: Mesh, c2w, K, near: float = RASTER_NEAR, texels: int = 8, scale: float = 1.0) -> torch.Tensor:
    """float32 [F]: the level of detail of every face of `mesh` in a pyramid over `texels` texels a leg, seen by the camera of
    `rasterize` (nerf_mip_lod): with g = scale * the leg in pixels of the right isosceles triangle that has the area of the
    rasteriser's snapped face, 0 where g >= texels - 1 (a texel of level 0 per pixel or fewer), rising linearly in g from level
    to level, L - 1 at the last one; 0 for a face the rasteriser drops.  scale > 1 sharpens, < 1 blurs.  No host read; F = 0:
    nothing is launched."""
    _check_mesh_tensors("face_lod", mesh)
    _, _, near, _, _ = check_raster_args(1, 1, near)
    mip_levels(texels)
    scale = check_lod_scale(scale)
    view, _keep = _raster_view(c2w, K)
    dev, V, F = mesh.verts.device, mesh.verts.shape[0], mesh.faces.shape[0]
    lod = torch.empty(F, dtype=torch.float32, device=dev)
    if F:
        N.check(N.lib().nerf_mip_lod(N.ptr(mesh.verts), V, N.ptr(mesh.faces), F, view, near, int(texels), scale, N.ptr(lod), N.stream()))
    return lod


def sample_texture_mip(pyramid: TexturePyramid, mesh: Mesh, face: torch.Tensor, bary: torch.Tensor, lod: torch.Tensor,
                       per_face: bool = False) -> torch.Tensor:
    """rgb float32 [n, 3]: the trilinear lookup of the pyramid at the surface samples (face, bary) of sample_texture and the level
    of detail `lod`, float32 [n], or with per_face [F] and read at the sample's face (face_lod's).  lod is clamped to [0, L - 1]
    (NaN reads level 0); an integral lod is exactly sample_texture on that level; a face outside [0, F) reads black
    (nerf_mip_sample)."""
    T = _check_pyramid("sample_texture_mip", pyramid, mesh)
    dev, F = mesh.verts.device, mesh.faces.shape[0]
    if not isinstance(per_face, bool):
        raise ValueError(f"sample_texture_mip: per_face must be a bool, got {per_face!r}")
    if not torch.is_tensor(face) or face.dtype != torch.int32 or face.dim() != 1 or not face.is_contiguous() or face.device != dev:
        raise ValueError("sample_texture_mip: face must be a contiguous int32 [n] tensor on the vertices' device")
    n = face.shape[0]
    if not torch.is_tensor(bary) or bary.dtype != torch.float32 or tuple(bary.shape) != (n, 2) or not bary.is_contiguous() \
            or bary.device != dev:
        raise ValueError(f"sample_texture_mip: bary must be a contiguous float32 [{n}, 2] tensor on the vertices' device")
    m = F if per_face else n
    if not torch.is_tensor(lod) or lod.dtype != torch.float32 or tuple(lod.shape) != (m,) or not lod.is_contiguous() or lod.device != dev:
        raise ValueError(f"sample_texture_mip: lod must be a contiguous float32 [{m}] tensor on the vertices' device")
    rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
    if n and F == 0:
        rgb.zero_()
    elif n:
        images = (C.c_void_p * len(pyramid.levels))(*[level.image.data_ptr() for level in pyramid.levels])
        N.check(N.lib().nerf_mip_sample(images, F, T, N.ptr(face), N.ptr(bary), N.ptr(lod), int(per_face), n, N.ptr(rgb), N.stream()))
    return rgb


def render_mesh_mip(mesh: Mesh, c2w, K, H: int, W: int, pyramid: TexturePyramid, background=None, near: float = RASTER_NEAR,
                    cull_backfaces: bool = False, mark=None, small_max: int = RASTER_SMALL_MAX, lod_scale: float = 1.0) -> MeshFrame:
    """render_mesh through a mip pyramid: rasterize, face_lod(scale=lod_scale) for the same camera, the
    trilinear lookup of sample_texture_mip at every pixel's (face, bary) with its face's level of detail, nerf_raster_shade.
    face, bary, depth and acc are render_mesh's; where every lod is 0 so is rgb.  mark: rasterize's stages, then "lod",
    "texture" and "shade"."""
    _check_mesh_tensors("render_mesh_mip", mesh)
    H, W, near, cull_backfaces, small_max = check_raster_args(H, W, near, cull_backfaces, small_max)
    T = _check_pyramid("render_mesh_mip", pyramid, mesh)
    lod_scale = check_lod_scale(lod_scale)
    dev, V, F = mesh.verts.device, mesh.verts.shape[0], mesh.faces.shape[0]
    bg, per_pixel = _raster_background(background, H, W, dev)
    face, bary, depth, acc, _ = rasterize(mesh, c2w, K, H, W, near, cull_backfaces, mark, small_max)
    if F == 0:
        rgb = (bg.reshape(H, W, 3) if per_pixel else bg.expand(H, W, 3)).clone()
        return MeshFrame(rgb, depth, acc, face, bary)
    _mark(mark, "lod")
    lod = face_lod(mesh, c2w, K, near, T, lod_scale)
    _mark(mark, "texture")
    looked_up = sample_texture_mip(pyramid, mesh, face.reshape(-1), bary.reshape(-1, 2), lod, per_face=True)
    rgb = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    _mark(mark, "shade")
    N.check(N.lib().nerf_raster_shade(N.ptr(face), N.ptr(bary), N.ptr(mesh.faces), V, F, None, N.ptr(looked_up), N.ptr(bg), per_pixel,
                                      H, W, N.ptr(rgb), N.stream()))
    return MeshFrame(rgb, depth, acc, face, bary)


def check_project_args(depth_tol, mode="blend", near=RASTER_NEAR, cos_min=PROJECT_COS_MIN, acc_min=0.5, chunk=CHUNK):
    """(depth_tol, mode number, near, cos_min, acc_min, chunk) as (float, int, float, float, float, int); ValueError for a
    depth_tol that is not a finite number >= 0 (there is no scale-free default: it is a length of the scene; Trainer.project_texture
    derives one from its scene box), a mode that is not "blend" or "best", a near that check_raster_args refuses, a cos_min or
    acc_min outside (0, 1], or a chunk that is not an int >= 1."""
    def real(x):
        return not isinstance(x, bool) and isinstance(x, numbers.Real) and math.isfinite(float(x))
    if not (real(depth_tol) and 0.0 <= float(depth_tol) <= float(np.finfo(np.float32).max)):
        raise ValueError(f"project depth_tol must be a finite number >= 0 in the scene's units, got {depth_tol!r}")
    if not isinstance(mode, str) or mode not in PROJECT_MODES:
        raise ValueError(f"project mode must be one of {sorted(PROJECT_MODES)}, got {mode!r}")
    near = check_raster_args(near=near)[2]
    for name, x in (("cos_min", cos_min), ("acc_min", acc_min)):
        if not (real(x) and 0.0 < float(np.float32(x)) <= 1.0):
            raise ValueError(f"project {name} must be a number in (0, 1], got {x!r}")
    if isinstance(chunk, bool) or not isinstance(chunk, numbers.Integral) or int(chunk) < 1:
        raise ValueError(f"project chunk must be an int >= 1, got {chunk!r}")
    return float(depth_tol), PROJECT_MODES[mode], near, float(cos_min), float(acc_min), int(chunk)


def project_texture(mesh: Mesh, images: torch.Tensor, c2w, K, texels: int = 8, depth_tol=None, mode: str = "blend",
                    fallback: Optional[Texture] = None, depth: Optional[torch.Tensor] = None, acc: Optional[torch.Tensor] = None,
                    near: float = RASTER_NEAR, cos_min: float = PROJECT_COS_MIN, acc_min: float = 0.5, chunk: int = CHUNK, mark=None):
    """(Texture, seen uint8 [H_atlas, W_atlas]): the atlas of bake_texture coloured from posed images (include/nerf_hip.h
    "view-projected texture").  images [n, H, W, 3] float32 on the mesh's device, c2w a stack of n poses and
    K as tsdf_views takes them.  Every texel is projected into every view; the view's bilinear colour there counts, with the
    weight cos(normal, direction to the camera) >= cos_min, only where the view's depth map, read at the nearest pixel, puts the
    surface no more than depth_tol (a length of the scene; required) in front of the texel.  mode "blend": the weighted mean over
    the views; "best": the view with the largest weight, the earlier one of equal weights.  depth, acc [n, H, W]: the maps of
    the views (a renderer's aux maps, depth not normalised); without them every view is rasterised (`rasterize` at `near`).  A
    texel no view sees takes the byte of `fallback`, a Texture of this mesh at these texels (bake_texture's, say), or 0; seen is
    1 where a view saw it.  PROJECT_MAX_VIEWS views per launch and `chunk` texels per launch; neither changes a bit.  F = 0 or
    n = 0: no projection kernel is launched.  No host read.  mark: _mark's hook ("rasterize" per view, "accumulate" per launch,
    then "finish" and "uv")."""
    T, (Wa, Ha, _, _) = check_texture_args(mesh, texels)
    tol, mode_id, near, cos_min, acc_min, chunk = check_project_args(depth_tol, mode, near, cos_min, acc_min, chunk)
    dev, V, F = mesh.verts.device, mesh.verts.shape[0], mesh.faces.shape[0]
    if not torch.is_tensor(images) or images.dtype != torch.float32 or images.dim() != 4 or images.shape[-1] != 3 \
            or not images.is_contiguous() or images.device != dev:
        raise ValueError("project_texture: images must be a contiguous float32 [n, H, W, 3] tensor on the vertices' device"
                         + (" (RGBA frames are not supported)" if torch.is_tensor(images) and images.dim() == 4 and images.shape[-1] == 4 else ""))
    n = images.shape[0]
    H, W = check_raster_args(int(images.shape[1]) if n else 1, int(images.shape[2]) if n else 1)[:2]
    views = tsdf_views(c2w, K) if n else np.zeros((0, 16), np.float32)
    if views.shape[0] != n:
        raise ValueError(f"project_texture: {n} images need {n} poses, got {views.shape[0]}")
    if (depth is None) != (acc is None):
        raise ValueError("project_texture: pass both depth and acc, or neither")
    for name, t in (("depth", depth), ("acc", acc)):
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32 or t.numel() != n * H * W or not t.is_contiguous()
                              or t.device != dev):
            raise ValueError(f"project_texture: {name} must be a contiguous float32 tensor of {n} x {H} x {W} elements on the vertices' device")
    fb = None
    if fallback is not None:
        if _check_texture("project_texture", fallback, mesh)[0] != T:
            raise ValueError(f"project_texture: the fallback has texels = {fallback.texels}, not {T}")
        fb = fallback.image
    uv = torch.empty(F, 3, 2, dtype=torch.float32, device=dev)
    if F == 0 or n == 0:                                                   # nothing is seen: the fallback, or black
        image = torch.zeros(Ha, Wa, 3, dtype=torch.uint8, device=dev) if fb is None else fb.clone()
        seen = torch.zeros(Ha, Wa, dtype=torch.uint8, device=dev)
    else:
        image = torch.empty(Ha, Wa, 3, dtype=torch.uint8, device=dev)
        seen = torch.empty(Ha, Wa, dtype=torch.uint8, device=dev)
    if F == 0:
        return Texture(image, uv, T), seen
    L = N.lib()
    P = Wa * Ha
    chunk = min(chunk, P)
    if n:
        state = torch.zeros(P, 4, dtype=torch.float32, device=dev)
        for s in range(0, n, PROJECT_MAX_VIEWS):
            m = min(PROJECT_MAX_VIEWS, n - s)
            if depth is None:
                both = []
                for k in range(s, s + m):
                    _mark(mark, "rasterize")
                    both.append(rasterize(mesh, views[k, :12].reshape(3, 4), _k_of(views[k]), H, W, near)[2:4])
                d, a = torch.stack([b[0] for b in both]), torch.stack([b[1] for b in both])
            else:
                d, a = depth.reshape(n, H * W)[s:s + m], acc.reshape(n, H * W)[s:s + m]
            v = np.ascontiguousarray(views[s:s + m])
            _mark(mark, "accumulate")
            for p0 in range(0, P, chunk):
                N.check(L.nerf_project_accumulate(N.ptr(mesh.verts), N.ptr(mesh.normals), V, N.ptr(mesh.faces), F, T, p0, min(chunk, P - p0),
                                                  v.ctypes.data_as(C.POINTER(C.c_float)), m, H, W, N.ptr(images[s:s + m]), N.ptr(d), N.ptr(a),
                                                  near, tol, cos_min, acc_min, mode_id, N.ptr(state), N.stream()))
        _mark(mark, "finish")
        N.check(L.nerf_project_finish(N.ptr(state), F, T, 0, P, mode_id, N.ptr(fb), N.ptr(image), N.ptr(seen), N.stream()))
    _mark(mark, "uv")
    N.check(L.nerf_texture_uv(F, T, N.ptr(uv), N.stream()))
    return Texture(image, uv, T), seen


def _k_of(view):
    """K [3, 3] of a nerf_tsdf_view row: its float32 fx, fy, cx, cy are exact as doubles, so tsdf_views gives the row back."""
    return np.array([[view[12], 0.0, view[14]], [0.0, view[13], view[15]], [0.0, 0.0, 1.0]], np.float64)


def _replace_file(path: str, data: bytes):
    tmp = path + ".tmp"
    with open(tmp, "wb") as fh:
        fh.write(data)
    os.replace(tmp, path)


def _png_chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def png_bytes(image: np.ndarray) -> bytes:
    """An 8-bit RGB PNG of a uint8 [H, W, 3] array, every row with filter type 0 (zlib and struct alone)."""
    H, W, _ = image.shape
    lines = np.zeros((H, 1 + 3 * W), np.uint8)
    lines[:, 1:] = image.reshape(H, 3 * W)
    return _PNG_MAGIC + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) \
        + _png_chunk(b"IDAT", zlib.compress(lines.tobytes(), 6)) + _png_chunk(b"IEND", b"")


def png_array(data: bytes) -> np.ndarray:
    """The inverse of png_bytes: uint8 [H, W, 3]; ValueError for anything but 8-bit RGB with filter type 0 throughout."""
    if data[:8] != _PNG_MAGIC:
        raise ValueError("not a PNG")
    pos, head, idat = 8, None, b""
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != zlib.crc32(kind + body):
            raise ValueError("PNG: bad chunk checksum")
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    if head is None or head[2:] != (8, 2, 0, 0, 0):
        raise ValueError("PNG: only 8-bit RGB without interlace")
    W, H = head[:2]
    lines = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 3 * W)
    if lines[:, 0].any():
        raise ValueError("PNG: only filter type 0")
    return lines[:, 1:].reshape(H, W, 3).copy()


def write_obj(path: str, mesh: Mesh, texture: Texture) -> str:
    """Wavefront OBJ with its material and texture: `path` (v, vn, one vt per face corner, `f a/t/a b/t/b c/t/c`, 1-based; floats
    with nine significant digits, which float32 survives), beside it the same name with the suffix .mtl (one material whose
    map_Kd names the image) and with .png (8-bit RGB, png_bytes).  Vertex colours are not written.  Each file is written under
    a temporary name, then renamed."""
    _check_texture("write_obj", texture, mesh)
    stem = os.path.splitext(path)[0]
    v = mesh.verts.detach().cpu().numpy().astype(np.float64)
    n = mesh.normals.detach().cpu().numpy().astype(np.float64)
    f = mesh.faces.detach().cpu().numpy().astype(np.int64) + 1
    uv = texture.uv.detach().cpu().numpy().astype(np.float64).reshape(-1, 2)
    out = [f"# texels {texture.texels}", f"mtllib {os.path.basename(stem)}.mtl", "usemtl atlas"]
    out += ["v %.9g %.9g %.9g" % tuple(r) for r in v]
    out += ["vn %.9g %.9g %.9g" % tuple(r) for r in n]
    out += ["vt %.9g %.9g" % tuple(r) for r in uv]
    out += ["f %d/%d/%d %d/%d/%d %d/%d/%d" % (a, 3 * k + 1, a, b, 3 * k + 2, b, c, 3 * k + 3, c) for k, (a, b, c) in enumerate(f)]
    _replace_file(stem + ".png", png_bytes(texture.image.detach().cpu().numpy()))
    _replace_file(stem + ".mtl", f"newmtl atlas\nKd 1 1 1\nmap_Kd {os.path.basename(stem)}.png\n".encode("ascii"))
    _replace_file(path, ("\n".join(out) + "\n").encode("ascii"))
    return path


def read_obj(path: str):
    """The inverse of write_obj: (Mesh without colours, Texture) as CPU tensors; only the layout write_obj produces."""
    with open(path) as fh:
        lines = [ln.split() for ln in fh]
    if not lines or lines[0][:2] != ["#", "texels"]:
        raise ValueError(f"{path}: not an OBJ of write_obj")
    T = int(lines[0][2])
    by = {k: [w[1:] for w in lines if w and w[0] == k] for k in ("v", "vn", "vt", "f", "mtllib")}
    verts = torch.tensor(np.array(by["v"], np.float64).reshape(-1, 3), dtype=torch.float32)
    normals = torch.tensor(np.array(by["vn"], np.float64).reshape(-1, 3), dtype=torch.float32)
    uv = torch.tensor(np.array(by["vt"], np.float64).reshape(-1, 3, 2), dtype=torch.float32)
    corners = np.array([[c.split("/") for c in w] for w in by["f"]], np.int64).reshape(-1, 3, 3)
    F = len(corners)
    if len(by["mtllib"]) != 1 or uv.shape[0] != F or normals.shape != verts.shape \
            or not np.array_equal(corners[:, :, 1].reshape(-1), np.arange(1, 3 * F + 1)) \
            or not np.array_equal(corners[:, :, 0], corners[:, :, 2]):
        raise ValueError(f"{path}: unexpected OBJ layout")
    here = os.path.dirname(path)
    with open(os.path.join(here, by["mtllib"][0][0])) as fh:
        maps = [ln.split()[1] for ln in fh if ln.startswith("map_Kd ")]
    if len(maps) != 1:
        raise ValueError(f"{path}: the material needs one map_Kd")
    with open(os.path.join(here, maps[0]), "rb") as fh:
        image = torch.from_numpy(png_array(fh.read()))
    faces = torch.from_numpy((corners[:, :, 0] - 1).astype(np.int32))
    return Mesh(verts, faces, normals), Texture(image, uv, T)
