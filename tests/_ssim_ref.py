"""Host mirror of csrc/metric.hip ssim_kernel (a helper module for the tests, not a conftest): numpy float32 with ONE rounding per
operation, in the operation order of the kernel (the library is built with -ffp-contract=off and `/` is correctly rounded).

  window, c1, c2   rounded to float32 first: they reach the kernel through c_float
  horizontal pass  acc = 0; acc = acc + w[k] q for k = 0 .. ws-1, on the five planes p, g, p p, g g, p g (each product rounded
                   before the multiply by w[k])
  vertical pass    the same order over rows
  closed form      mpp, mgg, mpg; vp = epp - mpp, vg, cov; v1 = 2 cov + c2, v2 = (vp + vg) + c2; cs = v1 / v2;
                   ssim = ((2 mpg + c1) v1) / (((mpp + mgg) + c1) v2)

The zero fill of a staged tile never reaches a valid output (x + k <= W - 1 and y + k <= H - 1 there), so the per-output values do
not depend on the tiling and the mirror needs none.  What depends on tiles, waves and atomics is the ORDER in which the device adds
the float32 outputs of one image in float64: `ssim_sums` gives the exact sum (math.fsum) and the first-order forward-error bound of
a float64 sum of n terms in any order, n 2^-53 sum |v| (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).

`mutate` plants one of two faults for the power tests of tests/test_ssim_ref_host.py (TX = 32 is the kernel's tile width):
  "tap"   the last window tap is dropped in the horizontal pass of the last valid column of every tile
  "halo"  the staged tile is one column short: its last column reads as zero (only full-width tiles use that column)
"""
import functools
import math

import numpy as np
import torch

from nerf_meets_mlx_amd import _native as N
from nerf_meets_mlx_amd.ops.metric import gaussian_window

f32, f64 = np.float32, np.float64
TX, TY, MAX_GRID, MAX_W, MAX_PLANES = 32, 8, 64, 33, 65535


def _pass(q, w, axis, drop=None):
    """acc = acc + w[k] q[.. + k] along `axis` (-1: columns, -2: rows) from acc = 0; `drop` [n_out] masks the last tap."""
    ws = w.size
    n_out = q.shape[axis] - ws + 1
    acc = np.zeros(q.shape[:axis] + (n_out,) + q.shape[q.ndim + axis + 1:], f32)
    for k in range(ws):
        term = w[k] * (q[..., k:k + n_out] if axis == -1 else q[..., k:k + n_out, :])
        if drop is not None and k == ws - 1:
            term = np.where(drop, f32(0.0), term)
        acc = acc + term
    assert acc.dtype == f32
    return acc


def _dropped_columns(OW, mutate):
    x = np.arange(OW)
    if mutate == "tap":
        return (x % TX == TX - 1) | (x == OW - 1)
    assert mutate == "halo", mutate
    return x % TX == TX - 1


def ssim_pixels(pred, gt, window, c1, c2, mutate=None):
    """(ssim, cs): float32 [..., H - ws + 1, W - ws + 1] of float32 planes [..., H, W]."""
    p, g = np.asarray(pred, f32), np.asarray(gt, f32)
    w, c1, c2 = np.asarray(window, f32), f32(c1), f32(c2)
    drop = _dropped_columns(p.shape[-1] - w.size + 1, mutate) if mutate else None
    with np.errstate(all="ignore"):
        mp, mg, epp, egg, epg = (_pass(_pass(q, w, -1, drop), w, -2) for q in (p, g, p * p, g * g, p * g))
        mpp, mgg, mpg = mp * mp, mg * mg, mp * mg
        vp, vg, cov = epp - mpp, egg - mgg, epg - mpg
        v1, v2 = f32(2.0) * cov + c2, (vp + vg) + c2
        cs = v1 / v2
        ssim = ((f32(2.0) * mpg + c1) * v1) / (((mpp + mgg) + c1) * v2)
    assert ssim.dtype == f32 and cs.dtype == f32
    return ssim, cs


def ssim_sums(pred, gt, window, c1, c2, mutate=None):
    """(sums [N, 2] float64, bound [N, 2] float64) of [N, C, H, W] images: column 0 is ssim, column 1 is cs."""
    maps = ssim_pixels(pred, gt, window, c1, c2, mutate)
    N_ = maps[0].shape[0]
    sums, bound = np.empty((N_, 2), f64), np.empty((N_, 2), f64)
    for col, m in enumerate(maps):
        for i in range(N_):
            v = m[i].reshape(-1).astype(f64).tolist()
            sums[i, col] = math.fsum(v)
            bound[i, col] = len(v) * 2.0 ** -53 * math.fsum(abs(t) for t in v)
    return sums, bound


def addends(shape, ws):
    """Outputs per image: C (H - ws + 1) (W - ws + 1)."""
    _, C_, H, W = shape
    return C_ * (H - ws + 1) * (W - ws + 1)


def tiles(shape, ws):
    _, _, H, W = shape
    return -(-(W - ws + 1) // TX) * -(-(H - ws + 1) // TY)


def constants(pred):
    """(c1, c2) as ops.metric.SSIM takes them from `pred`: L = (255 if max > 128 else 1) - (-1 if min < -0.5 else 0)."""
    L = (255 if float(pred.max()) > 128 else 1) - (-1 if float(pred.min()) < -0.5 else 0)
    return (0.01 * L) ** 2, (0.03 * L) ** 2


def window(ws, ref_quirks):
    return np.asarray(gaussian_window(ws, 1.5, ref_quirks), f64).astype(f32)


# ------------------------------------------------------------------------------------------------ the cases of both test files
# (N, C, H, W, w_size, range): range "unit" = [0, 1], "byte" = [0, 255] (L = 255), "signed" = [-1, 1] (L = 2)
CASES = {
    "tiles69": (1, 1, 189, 75, 11, "unit"),       # 3 x 23 = 69 tiles > 64 workgroups: second trip; 1-column and 3-row edge tiles
    "tiles66_w33": (1, 1, 207, 97, 33, "unit"),   # 3 x 22 = 66 tiles at the largest window and LDS footprint
    "images3": (3, 2, 37, 53, 5, "unit"),         # plane -> image attribution
    "one_tile_w33": (1, 1, 40, 64, 33, "unit"),   # exactly one full tile at w = 33
    "one_output": (1, 1, 33, 33, 33, "unit"),
    "w1": (2, 1, 12, 100, 1, "unit"),             # no halo
    "one_row": (1, 3, 11, 43, 11, "unit"),        # one output row, two tiles, the second 1 wide
    "byte": (3, 2, 37, 53, 5, "byte"),
    "signed": (3, 2, 37, 53, 5, "signed"),
}
assert tiles(CASES["tiles69"][:4], 11) == 69 and tiles(CASES["tiles66_w33"][:4], 33) == 66 and tiles(CASES["one_tile_w33"][:4], 33) == 1
assert tiles(CASES["one_row"][:4], 11) == 2 and addends(CASES["one_output"][:4], 33) == 1


def images(shape, rng_seed, value_range="unit"):
    """(pred, gt) float32 [N, C, H, W]: pred uniform in [0, 1], gt = clamp(pred + 0.1 s_i noise) with s_i = 1 + i / 2 for image i
    (the images' sums differ in the third digit), then mapped to the range."""
    rng = np.random.default_rng(rng_seed)
    pred = rng.uniform(0.0, 1.0, shape).astype(f32)
    scale = (f32(0.1) * (1.0 + 0.5 * np.arange(shape[0]))).astype(f32).reshape(-1, 1, 1, 1)
    gt = np.clip(pred + scale * rng.standard_normal(shape).astype(f32), f32(0.0), f32(1.0)).astype(f32)
    if value_range == "byte":
        pred, gt = pred * f32(255.0), gt * f32(255.0)
    elif value_range == "signed":
        pred, gt = f32(2.0) * pred - f32(1.0), f32(2.0) * gt - f32(1.0)
    else:
        assert value_range == "unit"
    return pred, gt


@functools.lru_cache(maxsize=None)
def case(name, ref_quirks):
    """The inputs and the mirror's result of one case, computed once per process (read-only: do not write into the arrays):
    dict(pred, gt, window, c1, c2, ws, sums, bound, n)."""
    N_, C_, H, W, ws, value_range = CASES[name]
    pred, gt = images((N_, C_, H, W), sorted(CASES).index(name) + 100, value_range)
    win = window(ws, ref_quirks)
    c1, c2 = constants(pred)
    sums, bound = ssim_sums(pred, gt, win, c1, c2)
    out = dict(pred=pred, gt=gt, window=win, c1=c1, c2=c2, ws=ws, sums=sums, bound=bound, n=addends(pred.shape, ws))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ raw caller
def poisoned_sums(n_images, device="cuda"):
    """[n_images, 2] float64 with 0xFF in every byte (NaN): the entry clears the buffer itself."""
    sums = torch.empty(n_images, 2, dtype=torch.float64, device=device)
    sums.view(torch.uint8).fill_(0xFF)
    return sums


def still_poisoned(sums):
    return bool((sums.view(torch.uint8) == 0xFF).all())


def ssim_sums_into(pred, gt, window, c1, c2, sums=None, shape=None, ws=None):
    """`nerf_ssim_sums` on device tensors -> the float64 [N, 2] `sums` tensor itself (poisoned first unless given).  `shape` and `ws`
    override what the tensors and the window say (for the refusals); `window` None passes NULL."""
    import ctypes as C
    n, ch, H, W = shape if shape is not None else pred.shape
    ws = ws if ws is not None else len(window)
    win = None if window is None else (C.c_float * len(window))(*[float(v) for v in window])
    if sums is None:
        sums = poisoned_sums(n, pred.device)
    N.check(N.lib().nerf_ssim_sums(N.ptr(pred), N.ptr(gt), n, ch, H, W, win, ws, float(c1), float(c2), N.ptr(sums), N.stream()))
    return sums
