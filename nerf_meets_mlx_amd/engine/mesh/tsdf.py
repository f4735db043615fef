"""TSDF fusion (include/nerf_hip.h "TSDF fusion").

  * `TSDFVolume(resolution, lo, hi, trunc)` fuses rendered depth / opacity maps of posed cameras into a truncated signed distance
    volume on the lattice of the volume stage (nerf_tsdf_integrate, 16 views per launch); `.volume()` is a volume for everything
    there at iso = 0.  `NGPTrainer.extract_mesh_tsdf` renders, fuses and meshes.
  * `tsdf_views(c2w, K)` packs poses and intrinsics into the float32 rows every camera entry of the library takes (the rasteriser,
    the projective bake and the mip pyramid's level of detail too); `_k_of` gives a row's K back."""
import math

import numpy as np
import torch

from ... import _native as N
from ._base import _box, _float_ptr, check_mesh_args
from ._checks import f32, need_int, need_real

TSDF_MAX_VIEWS = 16          # NERF_TSDF_MAX_VIEWS


def check_tsdf_args(trunc=None, acc_min=0.5, far=1.0, carve=True, min_views=1, H=1, W=1):
    """(trunc or None, acc_min, far, carve, min_views, H, W) as (float or None, float, float, bool, int, int, int); ValueError for
    a trunc or far that is not a finite number > 0 (trunc None: the volume's default), an acc_min outside (0, 1], a carve that is
    not a bool, a min_views that is not an int >= 1, or an H or W that is not an int in [1, 2^24]."""
    if trunc is not None:
        trunc = need_real(trunc, "tsdf trunc", "None or a finite number > 0", above=0.0)
    acc_min = need_real(acc_min, "tsdf acc_min", "a number in (0, 1]", above=0.0, most=1.0)
    far = need_real(far, "tsdf far", "a finite number > 0", above=0.0)
    if not isinstance(carve, bool):
        raise ValueError(f"tsdf carve must be a bool, got {carve!r}")
    min_views = need_int(min_views, "tsdf min_views", 1, want="an int >= 1")
    H, W = (need_int(x, f"tsdf {name}", 1, 1 << 24, "an int in [1, 2^24]") for name, x in (("H", H), ("W", W)))
    return trunc, acc_min, far, carve, min_views, H, W


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


def _k_of(view):
    """K [3, 3] of a nerf_tsdf_view row: its float32 fx, fy, cx, cy are exact as doubles, so tsdf_views gives the row back."""
    return np.array([[view[12], 0.0, view[14]], [0.0, view[13], view[15]], [0.0, 0.0, 1.0]], np.float64)


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
        self.trunc = f32(trunc)
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
            N.check(L.nerf_tsdf_integrate(N.ptr(self.D), N.ptr(self.Wt), N.ptr(self.flags), self.R, clo, chi,
                                          _float_ptr(views[s:s + m]), m, H, W, N.ptr(maps[0][s:s + m]),
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
