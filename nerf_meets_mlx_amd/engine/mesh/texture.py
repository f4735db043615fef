"""The texture stage: the atlas of a finished mesh and its mip pyramid (include/nerf_hip.h "texture atlas", "texture mip pyramid";
DESIGN.md sections 31, 34).

  * `bake_texture(query, mesh, texels)` bakes a texture atlas for a finished mesh, one field query per texel: a right triangle
    of `texels` texels a leg per face, two faces to a cell, gutters extrapolated so that bilinear lookups do not bleed;
    `sample_texture` looks it up at surface samples.  A separate step behind `extract`: the pipeline's keywords are what they
    were.
  * `build_mipmaps(texture, mesh)` reduces an atlas face by face into a `TexturePyramid` of complete textures and
    `sample_texture_mip` looks the pyramid up trilinearly at a level of detail (raster.face_lod's, say), so a face that covers one
    pixel is not point-sampled from 45 texels."""
import ctypes as C
from typing import NamedTuple

import torch

from ... import _native as N
from ._base import CHUNK, Mesh, _check_mesh_tensors, _clamped, _mark
from ._checks import need_int, need_tensor

TEXTURE_MAX_TEXELS = 64      # texels per triangle leg
TEXTURE_MAX_SIDE = 16384     # NERF_TEXTURE_MAX_SIDE
MIP_MAX_LEVELS = 6           # NERF_MIP_MAX_LEVELS: levels of a texture pyramid


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
    texels = need_int(texels, "texture texels", 2, TEXTURE_MAX_TEXELS)
    _, F = _check_mesh_tensors("texture", mesh)
    return texels, texture_layout(F, texels)


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
    chunk = _clamped(chunk, P)
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
    need_tensor(texture.image, f"{who}: image", torch.uint8, (lay[1], lay[0], 3), dev)
    need_tensor(texture.uv, f"{who}: uv", torch.float32, (F, 3, 2), dev)
    return T, lay


def _check_samples(who, face, bary, dev) -> int:
    """n of the surface samples of sample_texture and sample_texture_mip: face int32 [n] and bary float32 [n, 2] on `dev`."""
    need_tensor(face, f"{who}: face", torch.int32, (None,), dev, "[n]")
    n = face.shape[0]
    need_tensor(bary, f"{who}: bary", torch.float32, (n, 2), dev)
    return n


def sample_texture(texture: Texture, mesh: Mesh, face: torch.Tensor, bary: torch.Tensor, rows: bool = False):
    """rgb float32 [n, 3]: the bilinear lookup of the atlas at the surface samples (face [n] int32, bary [n, 2] float32 =
    the weights (wb, wc) of the face's second and third corner, clamped into the triangle); a face outside [0, F) reads black.
    With `rows` also the query rows [n, 11] of the very points, as bake_texture asks them (nerf_texture_sample)."""
    T, _ = _check_texture("sample_texture", texture, mesh)
    dev = mesh.verts.device
    n = _check_samples("sample_texture", face, bary, dev)
    rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
    out = torch.empty(n, 11, dtype=torch.float32, device=dev) if rows else None
    if n:
        N.check(N.lib().nerf_texture_sample(N.ptr(texture.image), N.ptr(mesh.verts), N.ptr(mesh.normals), mesh.verts.shape[0],
                                            N.ptr(mesh.faces), mesh.faces.shape[0], T, N.ptr(face), N.ptr(bary), n, N.ptr(rgb),
                                            N.ptr(out), N.stream()))
    return (rgb, out) if rows else rgb


class TexturePyramid(NamedTuple):
    levels: tuple                         # of Texture: levels[0] the atlas itself, levels[l] at mip_levels(texels)[l] texels a leg


def mip_levels(texels: int) -> tuple:
    """(T_0, ..., T_{L-1}): the texels per triangle leg of the levels of a pyramid over an atlas of `texels` (nerf_mip_levels; no
    device needed): T_{l+1} = (T_l + 1) // 2 while T_l > 2, at most MIP_MAX_LEVELS.  ValueError for texels outside
    [2, TEXTURE_MAX_TEXELS]."""
    need_int(texels, "mip texels", None, want=f"an int in [2, {TEXTURE_MAX_TEXELS}]")      # (the range is the library's to refuse)
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
        step = _clamped(chunk, P)
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
    n = _check_samples("sample_texture_mip", face, bary, dev)
    need_tensor(lod, "sample_texture_mip: lod", torch.float32, (F if per_face else n,), dev)
    rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
    if n and F == 0:
        rgb.zero_()
    elif n:
        images = (C.c_void_p * len(pyramid.levels))(*[level.image.data_ptr() for level in pyramid.levels])
        N.check(N.lib().nerf_mip_sample(images, F, T, N.ptr(face), N.ptr(bary), N.ptr(lod), int(per_face), n, N.ptr(rgb), N.stream()))
    return rgb
