"""Host mirrors of csrc/rays.hip (a helper module for the tests, not a conftest): ray generation, the NDC warp and the row gather
in numpy with ONE rounding per operation, in the operation order of the kernels (the library is built with -ffp-contract=off,
`/` and sqrtf are correctly rounded, subnormals are kept), so a kernel is compared with its mirror bit for bit.

  ray_gen      write_ray: the camera-space direction and its rotation are float64 (float64 K, the float32 rotation widened),
               summed left to right and rounded ONCE to float32; the unit view direction is float64 arithmetic on that float32
               direction, d * (1 / sqrt((x x + y y) + z z)), rounded ONCE to float32 (float64 `/` and sqrt are correctly rounded
               on the device too)
  ndc          ndc_kernel with the expression shapes as written: (2 near) / oz, ((-2) near) (1 / oz), dx / dz - ox / oz
  gather_rows  plain indexing; an index outside [0, n_src) gives a row of the quiet NaN 0x7FC00000

The raw callers below launch the C ABI entries of csrc/rays.hip into the middle of a buffer that holds SENTINEL in every word, with
PAD guard rows before and after: `unwritten(inner)` counts what the kernel skipped, `guards_intact(full)` what it wrote outside.
"""
import numpy as np
import torch

from nerf_meets_mlx_amd import _native as N
from nerf_meets_mlx_amd.rendering.ray import _host_cam
from tests._poison import SENTINEL, sentinel_, unwritten
from tests._render_ref import ELEMENTWISE_CAP  # noqa: F401  (one grid trip of every kernel here: grid_for(n, 256))

f32, f64 = np.float32, np.float64
PAD = 8
QNAN_BITS = 0x7FC00000


# ------------------------------------------------------------------------------------------------ mirrors
def ray_gen(p, W, K, c2w, near, far):
    """(rays [n, 11] float32, coords [n, 2] int64) of the flat pixel indices `p`."""
    p = np.asarray(p, np.int64).reshape(-1)
    K = np.asarray(K, f64).reshape(3, 3)
    c = np.asarray(c2w, f32)[:3, :4]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    r = c[:, :3].astype(f64)
    row = p // W
    col = p - row * W
    dx = (col.astype(f64) - cx) / fx
    dy = -(row.astype(f64) - cy) / fy
    dz = f64(-1.0)
    d = np.stack([(dx * r[a, 0] + dy * r[a, 1]) + dz * r[a, 2] for a in range(3)], -1).astype(f32)
    w = d.astype(f64)                                            # the float32 direction, widened: exact
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    with np.errstate(all="ignore"):
        inv = f64(1.0) / np.sqrt((x * x + y * y) + z * z)
        v = (w * inv[:, None]).astype(f32)
    rays = np.empty((p.size, 11), f32)
    rays[:, 0:3] = c[:, 3]
    rays[:, 3:6] = d
    rays[:, 6] = f32(near)
    rays[:, 7] = f32(far)
    rays[:, 8:11] = v
    assert rays.dtype == f32 and inv.dtype == f64
    return rays, np.stack([row, col], -1)


def ndc(rays, H, W, focal, near):
    """ndc_kernel in place on columns 0..5 of a [n, 11] float32 array (returned)."""
    assert rays.dtype == f32 and rays.ndim == 2 and rays.shape[1] == 11
    focal, near = f32(focal), f32(near)
    sx = -focal / (f32(0.5) * f32(W))
    sy = -focal / (f32(0.5) * f32(H))
    ox, oy, oz, dx, dy, dz = (rays[:, k].copy() for k in range(6))
    with np.errstate(all="ignore"):
        tn = -(near + oz) / dz
        ox = ox + tn * dx
        oy = oy + tn * dy
        oz = oz + tn * dz
        out = (sx * (ox / oz), sy * (oy / oz), f32(1.0) + (f32(2.0) * near) / oz,
               sx * (dx / dz - ox / oz), sy * (dy / dz - oy / oz), (f32(-2.0) * near) * (f32(1.0) / oz))
    for k, v in enumerate(out):
        assert v.dtype == f32
        rays[:, k] = v
    return rays


def gather_rows(src, idx):
    """out[i] = src[idx[i]] of a [n_src, C] float32 array; rows whose index is outside [0, n_src) are the quiet NaN."""
    src = np.asarray(src, f32)
    idx = np.asarray(idx, np.int64).reshape(-1)
    ok = (idx >= 0) & (idx < src.shape[0])
    out = np.full((idx.size, src.shape[1]), QNAN_BITS, np.uint32).view(f32)
    out[ok] = src[idx[ok]]
    return out


# ------------------------------------------------------------------------------------------------ guarded buffers
def guarded(rows, cols, device, dtype=torch.float32):
    """(full, inner): a SENTINEL-filled [rows + 2 PAD, cols] buffer and its middle [rows, cols]."""
    full = sentinel_(torch.empty(rows + 2 * PAD, cols, dtype=dtype, device=device))
    return full, full[PAD:PAD + rows]


def guards_intact(full):
    """The PAD rows before and after the middle still hold SENTINEL in every 32-bit word."""
    words = full.shape[1] * full.element_size() // 4
    return unwritten(full[:PAD]) == PAD * words and unwritten(full[full.shape[0] - PAD:]) == PAD * words


def from_host(a, device):
    """A guarded device copy of a host [rows, cols] float32 array: (full, inner)."""
    a = np.ascontiguousarray(a, f32)
    full, inner = guarded(a.shape[0], a.shape[1], device)
    inner.copy_(torch.from_numpy(a))
    return full, inner


def bits(t):
    """The 32-bit words of a tensor as a host uint32 array."""
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ raw callers
def ray_gen_into(idx, n, H, W, K, c2w, near, far, want_coords, device="cuda"):
    """`nerf_ray_gen` (idx None = NULL: all H W pixels) -> (rays_full, rays, coords_full or None, coords or None)."""
    r_full, r = guarded(n, 11, device)
    c_full, c = guarded(n, 2, device, torch.int64) if want_coords else (None, None)
    Kc, cc = _host_cam(K, c2w)
    N.check(N.lib().nerf_ray_gen(N.ptr(idx), n, H, W, Kc, cc, float(near), float(far), N.ptr(r), N.ptr(c), N.stream()))
    return r_full, r, c_full, c


def ndc_into(rays, H, W, focal, near, device="cuda"):
    """`nerf_ndc_rays` in place on a guarded copy of the host array `rays` [n, 11] -> (full, inner)."""
    full, inner = from_host(rays, device)
    N.check(N.lib().nerf_ndc_rays(N.ptr(inner), inner.shape[0], int(H), int(W), float(focal), float(near), N.stream()))
    return full, inner


def gather_rows_into(src, idx, device="cuda"):
    """`nerf_gather_rows` of a device [n_src, C] tensor `src` (any view of a larger buffer) -> (full, inner)."""
    n, ch = idx.numel(), src.shape[1]
    full, inner = guarded(n, ch, device)
    N.check(N.lib().nerf_gather_rows(N.ptr(src), src.shape[0], N.ptr(idx), n, ch, N.ptr(inner), N.stream()))
    return full, inner


def pixel_permutation_into(n, domain, seed, offset=0, device="cuda"):
    """`nerf_pixel_permutation` -> (full [n + 2 PAD, 1] int64, inner)."""
    full, inner = guarded(n, 1, device, torch.int64)
    N.check(N.lib().nerf_pixel_permutation(N.ptr(inner), n, domain, seed & ((1 << 64) - 1), offset, N.stream()))
    return full, inner


def sample_batch_into(n, H, W, seed, offset, K, c2w, near, far, image, want_idx=True):
    """`nerf_sample_batch` ([H W, 3] image) or `nerf_sample_batch_rgba` ([H W, 4]) -> {"rays", "target", "idx"}: (full, inner)."""
    ch = image.shape[1]
    fn = {3: N.lib().nerf_sample_batch, 4: N.lib().nerf_sample_batch_rgba}[ch]
    o = {"rays": guarded(n, 11, image.device), "target": guarded(n, ch, image.device)}
    if want_idx:
        o["idx"] = guarded(n, 1, image.device, torch.int64)
    Kc, cc = _host_cam(K, c2w)
    N.check(fn(n, H, W, seed & ((1 << 64) - 1), offset, Kc, cc, float(near), float(far), N.ptr(image), N.ptr(o["rays"][1]),
               N.ptr(o["target"][1]), N.ptr(o["idx"][1]) if want_idx else None, N.stream()))
    return o


# ------------------------------------------------------------------------------------------------ shared inputs
def adversarial_camera():
    """(H, W, K float64, c2w float32 [3, 4]): W != H, both odd; fx != fy; non-integer cx != W/2, cy != H/2; K entries that float32
    cannot hold; a 3x3 part that is neither orthonormal nor symmetric; a translation that is not zero."""
    H, W = 37, 53
    K = np.array([[61.3 + 1e-9, 0.0, 24.7 + 1e-10], [0.0, 47.9 - 1e-9, 20.3 + 1e-11], [0.0, 0.0, 1.0]], f64)
    c2w = np.array([[0.83, -0.31, 0.52, 1.25], [0.17, 1.07, -0.44, -2.5], [-0.61, 0.29, 0.71, 3.75]], f32)
    assert all(float(f32(K[i, j])) != K[i, j] for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))
    return H, W, K, c2w


def ndc_inputs(kind, n, seed=0):
    """[n, 11] float32 host rays for the NDC tests; columns 6..10 hold SENTINEL.
    random   the rays of the older test (origins about z = -4, dz <= -0.5)
    near     origins already on the near plane: oz == -near, so tn is +-0
    tiny_dz  |dz| from 1 down to 1e-30, every eighth one exactly +-0, every eighth dx times 1e9: infinities and NaN
    subnormal  dx in the float32 subnormal range"""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g)
    o[:, 2] -= 4.0
    d = torch.randn(n, 3, generator=g)
    d[:, 2] = -d[:, 2].abs() - 0.5
    o, d = o.numpy().copy(), d.numpy().copy()
    i = np.arange(n)
    if kind == "near":
        o[:, 2] = -1.0
    elif kind == "tiny_dz":
        d[:, 2] = (-1.0) ** i * 10.0 ** (-30.0 * ((i % 97) / 96.0))
        d[i % 8 == 3, 2] = 0.0
        d[i % 16 == 11, 2] = -0.0
        d[i % 8 == 5, 0] *= 1e9                                  # dx / dz and tn dx overflow: infinite o'x, NaN d'x
    elif kind == "subnormal":
        d[:, 0] = ((-1.0) ** i * (1 + i % 1000) * 2.0 ** -149 * 2.0 ** (i % 12)).astype(f32)
        assert (np.abs(d[:, 0]) < np.finfo(f32).tiny).all() and (d[:, 0] != 0).all()
    else:
        assert kind == "random"
    rays = np.full((n, 11), SENTINEL, np.uint32).view(f32)
    rays[:, 0:3], rays[:, 3:6] = o, d
    return rays
