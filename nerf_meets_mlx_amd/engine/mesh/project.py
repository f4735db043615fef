"""The projective bake (include/nerf_hip.h "view-projected texture").

  * `project_texture(mesh, images, c2w, K, texels, depth_tol)` colours the atlas of the texture stage from posed pictures: every
    texel takes what the views saw of it where the mesh's own depth map of the view (the rasteriser's, unless the caller brings
    one) says it is visible, blended by the cosine or from the best view, and a fallback texture elsewhere."""
from typing import Optional

import numpy as np
import torch

from ... import _native as N
from ._base import CHUNK, Mesh, _clamped, _float_ptr, _mark
from ._checks import F32_MAX, is_tensor, need_int, need_real
from .raster import RASTER_NEAR, check_raster_args, rasterize
from .texture import Texture, _check_texture, check_texture_args
from .tsdf import _k_of, tsdf_views

PROJECT_MAX_VIEWS = 16       # NERF_PROJECT_MAX_VIEWS: views per launch of the projective bake
PROJECT_MODES = {"blend": 0, "best": 1}   # NERF_PROJECT_BLEND / NERF_PROJECT_BEST
PROJECT_COS_MIN = 0.05       # the projective bake's default grazing limit: the best of the sweep of DESIGN.md section 33
PROJECT_DEPTH_TOL_CELLS = 4.0  # Trainer.project_texture's default depth_tol in spacings of a 256^3 lattice on its scene box (section 33)


def check_project_args(depth_tol, mode="blend", near=RASTER_NEAR, cos_min=PROJECT_COS_MIN, acc_min=0.5, chunk=CHUNK):
    """(depth_tol, mode number, near, cos_min, acc_min, chunk) as (float, int, float, float, float, int); ValueError for a
    depth_tol that is not a finite number >= 0 (there is no scale-free default: it is a length of the scene; Trainer.project_texture
    derives one from its scene box), a mode that is not "blend" or "best", a near that check_raster_args refuses, a cos_min or
    acc_min outside (0, 1], or a chunk that is not an int >= 1."""
    depth_tol = need_real(depth_tol, "project depth_tol", "a finite number >= 0 in the scene's units", least=0.0, most=F32_MAX)
    if not isinstance(mode, str) or mode not in PROJECT_MODES:
        raise ValueError(f"project mode must be one of {sorted(PROJECT_MODES)}, got {mode!r}")
    near = check_raster_args(near=near)[2]
    cos_min, acc_min = (need_real(x, f"project {name}", "a number in (0, 1]", above=0.0, most=1.0, as_f32=True)
                        for name, x in (("cos_min", cos_min), ("acc_min", acc_min)))
    return depth_tol, PROJECT_MODES[mode], near, cos_min, acc_min, need_int(chunk, "project chunk", 1, want="an int >= 1")


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
    if not is_tensor(images, torch.float32, (None, None, None, 3), dev):
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
        if t is not None and (not is_tensor(t, torch.float32, None, dev) or t.numel() != n * H * W):
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
    chunk = _clamped(chunk, P)
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
            v = _float_ptr(views[s:s + m])
            _mark(mark, "accumulate")
            for p0 in range(0, P, chunk):
                N.check(L.nerf_project_accumulate(N.ptr(mesh.verts), N.ptr(mesh.normals), V, N.ptr(mesh.faces), F, T, p0, min(chunk, P - p0),
                                                  v, m, H, W, N.ptr(images[s:s + m]), N.ptr(d), N.ptr(a),
                                                  near, tol, cos_min, acc_min, mode_id, N.ptr(state), N.stream()))
        _mark(mark, "finish")
        N.check(L.nerf_project_finish(N.ptr(state), F, T, 0, P, mode_id, N.ptr(fb), N.ptr(image), N.ptr(seen), N.stream()))
    _mark(mark, "uv")
    N.check(L.nerf_texture_uv(F, T, N.ptr(uv), N.stream()))
    return Texture(image, uv, T), seen
