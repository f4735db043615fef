"""The volume stage: a field's density on the lattice, its mesh, and the filters of the volume in between (include/nerf_hip.h "mesh
extraction", "connected components", "morphological opening"; DESIGN.md sections 14, 17, 18).

  * `marching_cubes(volume, iso, lo, hi)` turns a float32 [R, R, R] device volume (vol[k, j, i] at the cell centres
    lo + (i + 0.5) h of the box) into a welded, consistently oriented triangle mesh: nerf_mesh_count, one read of (V, F) to the
    host, nerf_mesh_write_vertices, nerf_mesh_write_faces.
  * `Trainer.density_volume` / `Trainer.extract_mesh` (engine/trainer.py) sample the field on that lattice with its fused query
    (nerf_mesh_points, the query, nerf_occ_merge_ex with decay 0) and colour the vertices by a query along -normal.
  * `connected_components(volume, iso)` labels the 6-connected components of {v > iso}; `filter_components` sets the small ones
    (or all but the largest) to `iso`, which removes their pieces from the mesh and leaves the rest of it bit for bit.
  * `erode(volume, iso, radius)` takes `radius` 6-neighbour layers off {v > iso} (the box faces erode too), which cuts the thin
    bridges that tie a floater to the surface; `reconstruct(volume, kept, iso, radius)` grows what was kept back inside
    {v > iso} by exactly `radius` geodesic steps; `open_components` is erode -> filter_components on the core -> reconstruct.
  * `extract(...)` is density_volume -> `filter_volume` (the opening with opening_radius > 0, where `min_component` counts core
    voxels, else the plain filter, else nothing) -> `mesh_volume`: marching cubes, the surface stage, the colour query.
    `check_volume_options` and surface.check_surface_options are the one check of its post-processing keywords."""
from typing import NamedTuple, Optional

import torch

from ... import _native as N
from ._base import CHUNK, Mesh, _box, _clamped, _mark, check_mesh_args
from ._checks import is_tensor, need_int
from .surface import _simplify, _smooth, check_smooth_params, check_surface_options

MAX_OPENING_RADIUS = 16      # NERF_MORPH_MAX_RADIUS
RELU, EXP = 0, 1             # NERF_OCC_RELU / NERF_OCC_EXP


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
    chunk = _clamped(chunk, n3)
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
    if not is_tensor(volume, torch.float32, (None,) * 3) or not (volume.shape[0] == volume.shape[1] == volume.shape[2]):
        raise ValueError(f"{who}: volume must be a contiguous float32 [R, R, R] tensor")
    return check_mesh_args(volume.shape[0], lo, hi, iso)


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
    min_component = need_int(min_component, "min_component", 0, int(resolution) ** 3)
    if not isinstance(largest_only, bool):
        raise ValueError(f"largest_only must be a bool, got {largest_only!r}")
    return min_component, largest_only


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
        if not is_tensor(t, dt, shape, volume.device):
            raise ValueError("filter_components: components do not belong to this volume")
    out = torch.empty_like(volume)
    _mark(mark, "filter")
    N.check(N.lib().nerf_ccl_filter(N.ptr(volume), N.ptr(c.labels), N.ptr(c.sizes), N.ptr(c.stats), R, iso, min_component,
                                    int(largest_only), N.ptr(out), N.stream()))
    return out


def check_opening_args(opening_radius) -> int:
    """opening_radius as an int; ValueError for a bool, a non-integral value or one outside [0, MAX_OPENING_RADIUS] (0: no
    opening)."""
    return need_int(opening_radius, "opening_radius", 0, MAX_OPENING_RADIUS)


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
    if not is_tensor(kept, volume.dtype, tuple(volume.shape), volume.device):
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


def extract(query, activation: int, resolution: int, threshold: float, lo, hi, colors: bool = True, device="cuda",
            min_component: int = 0, largest_only: bool = False, opening_radius: int = 0, simplify_grid: int = 0,
            simplify_placement: str = "quadric", smooth_iterations: int = 0, smooth_lambda: float = 0.5,
            smooth_mu: float = -0.53) -> Mesh:
    """density_volume -> (with opening_radius > 0: open_components; else with min_component > 1 or largest_only:
    filter_components) -> marching_cubes at `threshold` -> (with smooth_iterations > 0: smooth) -> (with simplify_grid > 0:
    simplify on that grid of the box) -> (optionally) vertex colours, queried on the final mesh's rows: the field is asked once
    per vertex that is kept.  With opening_radius > 0 `min_component` counts core voxels (open_components).  With the defaults
    none of them is called."""
    R = check_mesh_args(resolution, lo, hi, threshold)[0]
    volume_options = check_volume_options(min_component, largest_only, opening_radius, R)
    surface_options = check_surface_options(simplify_grid, simplify_placement, smooth_iterations, smooth_lambda, smooth_mu)
    vol = density_volume(query, activation, resolution, lo, hi, device=device)
    return mesh_volume(query, filter_volume(vol, threshold, *volume_options), threshold, lo, hi, colors, *surface_options)


def check_volume_options(min_component, largest_only, opening_radius, resolution: int):
    """(min_component, largest_only, opening_radius) as (int, bool, int): the volume-stage keywords of extract, Trainer.extract_mesh
    and NGPTrainer.extract_mesh_tsdf, checked in this order by check_component_args and check_opening_args."""
    return (*check_component_args(min_component, largest_only, resolution), check_opening_args(opening_radius))


def filter_volume(vol: torch.Tensor, iso: float, min_component: int, largest_only: bool, opening_radius: int) -> torch.Tensor:
    """The volume stage on checked options: open_components with opening_radius > 0, else filter_components with
    min_component > 1 or largest_only, else `vol` itself."""
    if opening_radius > 0:
        return open_components(vol, iso, opening_radius, min_component, largest_only)
    if min_component > 1 or largest_only:
        return filter_components(vol, iso, min_component, largest_only)
    return vol


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
