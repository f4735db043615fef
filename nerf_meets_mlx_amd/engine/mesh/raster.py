"""The rasteriser and the two renderers (include/nerf_hip.h "mesh rendering", "texture mip pyramid"; DESIGN.md sections 32, 34).

  * `rasterize(mesh, c2w, K, H, W)` finds the face every pixel centre of a posed pinhole camera sees, its barycentrics and its
    depth, by exact integer coverage and one 64-bit atomicMin per covered pixel; `render_mesh` shades that with the vertex
    colours or through `sample_texture` into a `MeshFrame`, so a mesh can be compared with the held-out frame and with the
    field's render in image space (`Trainer.mesh_psnr`).
  * `face_lod` gives every face a level of detail from its footprint on a camera's screen, and `render_mesh_mip` looks a
    `TexturePyramid` up trilinearly there through `sample_texture_mip`.
  * `_render` is the one body of both renderers: the checks, the background, `rasterize`, the lookup its caller hands in,
    nerf_raster_shade."""
from typing import NamedTuple, Optional

import torch

from ... import _native as N
from ._base import Mesh, _check_mesh_tensors, _float_ptr, _mark
from ._checks import F32_MAX, need_int, need_real
from .texture import Texture, TexturePyramid, _check_pyramid, _check_texture, mip_levels, sample_texture, sample_texture_mip
from .tsdf import tsdf_views

RASTER_MAX_SIDE = 16384      # image height and width of the mesh renderer
RASTER_SMALL_MAX = 16        # NERF_RASTER_SMALL_MAX
RASTER_NEAR = 0.01           # the mesh renderer's default near plane


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
    H, W = (need_int(x, f"raster {name}", 1, RASTER_MAX_SIDE) for name, x in (("H", H), ("W", W)))
    near = need_real(near, "raster near", "a finite number > 0", above=0.0, most=F32_MAX, as_f32=True)
    if not isinstance(cull_backfaces, bool):
        raise ValueError(f"raster cull_backfaces must be a bool, got {cull_backfaces!r}")
    return H, W, near, cull_backfaces, need_int(small_max, "raster small_max", 0, 1 << 30, "an int in [0, 2^30]")


def _raster_view(c2w, K):
    views = tsdf_views(c2w, K)
    if views.shape[0] != 1:
        raise ValueError(f"raster: need one camera, got a stack of {views.shape[0]}")
    return _float_ptr(views[0]), views


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


def check_lod_scale(scale) -> float:
    """`scale` as a float; ValueError unless it is a finite number > 0 (as a float32)."""
    return need_real(scale, "mip lod scale", "a finite number > 0", above=0.0, most=F32_MAX, as_f32=True)


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


def _render(who, mesh, c2w, K, H, W, prepare, background, near, cull_backfaces, mark, small_max, visibility=None) -> MeshFrame:
    """The body of render_mesh, render_mesh_mip and render_mesh_rays.  prepare(): the caller's own checks, made between the raster
    arguments and the background; it returns None for the vertex colours or lookup(face [H W], bary [H W, 2], near) -> rgb [H W, 3],
    which is called behind rasterize when there are faces and calls `mark` for its own stages.  visibility(near) -> (face, bary,
    depth, acc, ...) stands in for rasterize (raycast.py's raycast_frame); None: rasterize."""
    _check_mesh_tensors(who, mesh)
    H, W, near, cull_backfaces, small_max = check_raster_args(H, W, near, cull_backfaces, small_max)
    lookup = prepare()
    dev, V, F = mesh.verts.device, mesh.verts.shape[0], mesh.faces.shape[0]
    bg, per_pixel = _raster_background(background, H, W, dev)
    if visibility is None:
        face, bary, depth, acc, _ = rasterize(mesh, c2w, K, H, W, near, cull_backfaces, mark, small_max)
    else:
        face, bary, depth, acc, _ = visibility(near)
    if F == 0:
        rgb = (bg.reshape(H, W, 3) if per_pixel else bg.expand(H, W, 3)).clone()
        return MeshFrame(rgb, depth, acc, face, bary)
    looked_up = lookup(face.reshape(-1), bary.reshape(-1, 2), near) if lookup is not None else None
    rgb = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    _mark(mark, "shade")
    N.check(N.lib().nerf_raster_shade(N.ptr(face), N.ptr(bary), N.ptr(mesh.faces), V, F, None if lookup is not None else N.ptr(mesh.colors),
                                      N.ptr(looked_up), N.ptr(bg), per_pixel, H, W, N.ptr(rgb), N.stream()))
    return MeshFrame(rgb, depth, acc, face, bary)


def render_mesh(mesh: Mesh, c2w, K, H: int, W: int, texture: Optional[Texture] = None, background=None, near: float = RASTER_NEAR,
                cull_backfaces: bool = False, mark=None, small_max: int = RASTER_SMALL_MAX) -> MeshFrame:
    """The picture of `mesh` from the camera of `rasterize`: with `texture` every covered pixel looks the atlas up at its
    (face, bary) through sample_texture; without one it takes the barycentric sum of mesh.colors (ValueError if there are none).
    Empty pixels take `background`: None is white, else one colour or one per pixel as Trainer.render_frame.  One sample at the
    pixel centre; no antialiasing.  mark: rasterize's stages, then "texture" (with one) and "shade"."""
    def lookup(face, bary, near):
        _mark(mark, "texture")
        return sample_texture(texture, mesh, face, bary)

    def prepare():
        if texture is not None:
            _check_texture("render_mesh", texture, mesh)
            return lookup
        if mesh.colors is None:
            raise ValueError("render_mesh: a mesh without colors needs a texture")

    return _render("render_mesh", mesh, c2w, K, H, W, prepare, background, near, cull_backfaces, mark, small_max)


def render_mesh_mip(mesh: Mesh, c2w, K, H: int, W: int, pyramid: TexturePyramid, background=None, near: float = RASTER_NEAR,
                    cull_backfaces: bool = False, mark=None, small_max: int = RASTER_SMALL_MAX, lod_scale: float = 1.0) -> MeshFrame:
    """render_mesh through a mip pyramid: rasterize, face_lod(scale=lod_scale) for the same camera, the
    trilinear lookup of sample_texture_mip at every pixel's (face, bary) with its face's level of detail, nerf_raster_shade.
    face, bary, depth and acc are render_mesh's; where every lod is 0 so is rgb.  mark: rasterize's stages, then "lod",
    "texture" and "shade"."""
    def prepare():
        T, scale = _check_pyramid("render_mesh_mip", pyramid, mesh), check_lod_scale(lod_scale)

        def lookup(face, bary, near):
            _mark(mark, "lod")
            lod = face_lod(mesh, c2w, K, near, T, scale)
            _mark(mark, "texture")
            return sample_texture_mip(pyramid, mesh, face, bary, lod, per_face=True)
        return lookup

    return _render("render_mesh_mip", mesh, c2w, K, H, W, prepare, background, near, cull_backfaces, mark, small_max)
