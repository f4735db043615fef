"""What every stage of the mesh layer shares: the `Mesh` tuple and the check of its tensors, the lattice arguments (resolution, box,
iso level), the stage hook `_mark`, and the small conversions for the C entry points."""
import ctypes as C
import math
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from ._checks import is_tensor, need_int, need_real, need_tensor

MAX_RES = 512                # NERF_MESH_MAX_RES
CHUNK = 1 << 19              # lattice points (or vertices) per query, as OccupancyGrid.update
MESH_MAX_ITEMS = 1 << 24  # vertices, faces


class Mesh(NamedTuple):
    verts: torch.Tensor                   # [V, 3] float32
    faces: torch.Tensor                   # [F, 3] int32, counter-clockwise seen from outside
    normals: torch.Tensor                 # [V, 3] float32, unit or 0
    colors: Optional[torch.Tensor] = None  # [V, 3] float32 in [0, 1], or None


def check_mesh_args(resolution, lo: Sequence[float], hi: Sequence[float], iso=0.0):
    """(R, lo [3], hi [3], iso) as (int, float lists, float); ValueError for R outside [2, MAX_RES], a box with lo >= hi or a
    non-finite corner, or a non-finite iso."""
    resolution = need_int(resolution, "mesh resolution", 2, MAX_RES)
    lo = [float(x) for x in lo]
    hi = [float(x) for x in hi]
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError(f"mesh box: lo and hi need 3 coordinates each, got {lo!r}, {hi!r}")
    if not all(math.isfinite(a) and math.isfinite(b) and a < b for a, b in zip(lo, hi)):
        raise ValueError(f"mesh box: need finite lo < hi on every axis, got lo={lo!r}, hi={hi!r}")
    return resolution, lo, hi, need_real(iso, "mesh iso level")


def _box(lo, hi):
    return (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)


def _float_ptr(a):
    """float* of a host float32 array (a view is copied); the pointer keeps the array alive."""
    return np.ascontiguousarray(a).ctypes.data_as(C.POINTER(C.c_float))


def _clamped(chunk, n: int) -> int:
    """A chunk length for n >= 1 items: `chunk` as an int, clamped to [1, n]."""
    return max(1, min(int(chunk), n))


def _mark(mark, stage):
    """The stage hook of connected_components, filter_components, erode, reconstruct, _open_components, _simplify and _smooth:
    mark(stage) just ahead of the stage's first C call (tools/ngp_mesh.py records a device event there).  None: nothing is
    called."""
    if mark is not None:
        mark(stage)


def _rows(points) -> int:
    """The rows of a [n, k] tensor; 0 for anything else, which the caller's need_tensor then refuses by name."""
    return points.shape[0] if torch.is_tensor(points) and points.dim() == 2 else 0


def _query_in_order(points, order, outs, run, mark=None):
    """The shell of the point queries (MeshIndex, MeshBVH, MeshWinding): run(points, *outs) fills the empty tensors `outs`, one row
    per point (stage "query").  With a permutation `order` (int64 [n], or a function of the points, computed inside stage "sort")
    run gets the points in that order and the answers are scattered back, out[order] = value (stage "scatter").  Returns `outs`,
    at once and without calling anything when there is no point."""
    if points.shape[0] == 0:
        return outs
    if order is None:
        _mark(mark, "query")
        run(points, *outs)
        return outs
    _mark(mark, "sort")
    if callable(order):
        order = order(points)
    points, sorted_outs = points[order].contiguous(), tuple(torch.empty_like(o) for o in outs)
    _mark(mark, "query")
    run(points, *sorted_outs)
    _mark(mark, "scatter")
    for o, s in zip(outs, sorted_outs):
        o[order] = s
    return outs


def _check_mesh_tensors(who, mesh):
    """(V, F) of a Mesh whose tensors are contiguous verts float32 [V, 3], faces int32 [F, 3], normals float32 [V, 3] and colors
    None or float32 [V, 3] on one device, with V, F <= 2^24; ValueError otherwise (check_simplify_args, check_smooth_args,
    check_texture_args)."""
    if not isinstance(mesh, Mesh):
        raise ValueError(f"{who}: need an engine.mesh.Mesh, got {type(mesh).__name__}")
    need_tensor(mesh.verts, f"{who}: verts", torch.float32, (None, 3), shown="[V, 3]")
    V, dev = mesh.verts.shape[0], mesh.verts.device
    need_tensor(mesh.faces, f"{who}: faces", torch.int32, (None, 3), dev, "[F, 3]")
    need_tensor(mesh.normals, f"{who}: normals", torch.float32, (V, 3), dev, "[V, 3]")
    if mesh.colors is not None and not is_tensor(mesh.colors, torch.float32, (V, 3), dev):
        raise ValueError(f"{who}: colors must be None or a contiguous float32 [V, 3] tensor on the vertices' device")
    F = mesh.faces.shape[0]
    if V > MESH_MAX_ITEMS or F > MESH_MAX_ITEMS:
        raise ValueError(f"{who}: at most 2^24 vertices and faces, got {V} and {F}")
    return V, F
