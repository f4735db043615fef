"""Host reference of the level-weight (`_lw`) entries of the hash grid (a helper module for the tests, not a conftest).

tests/_hashgrid_ref.py is the bit-exact float32 emulation of the entries without weights; the weighted forms add ONE float32
multiply each, in the operation order include/nerf_hip.h states ("Level weights"):
  encode    feature (l, f) = w[l] * interp_l,f; a level with w[l] == 0 is not read and gives exactly +0
  addends   g = w[l] * d_out[., l, f], then the addend formula with g in place of d_out; a level with w[l] == 0 has no addends
"""
import numpy as np

from tests import _hashgrid_ref as R

f32 = np.float32


def weights(w):
    w = np.asarray(w, dtype=f32)
    assert np.isfinite(w).all() and (w >= 0).all() and (w <= 1).all()
    return w


def encode(p, tables, res, w):
    """[M, L F] weighted hash features; tables [L, T, F].  The tables of masked levels are never looked at."""
    w = weights(w)
    tables = np.array(tables, dtype=f32, copy=True)
    L, T, F = tables.shape
    tables[w == 0] = 0                                       # not read: whatever they hold (NaN included) cannot matter
    out = R.encode(p, tables, res).reshape(p.shape[0], L, F)
    with np.errstate(invalid="ignore"):
        out = (w[None, :, None] * out).astype(f32)           # one float32 multiply (1 * x == x bit for bit)
    out[:, w == 0, :] = f32(0.0)                             # exactly +0, also for NaN positions
    return out.reshape(p.shape[0], L * F)


def premultiplied(d_out, w, L, F):
    """d_out [M, L F] with every level column multiplied by w[l] in float32 (what the entry without weights is fed)."""
    d = np.asarray(d_out, dtype=f32).reshape(-1, L, F)
    with np.errstate(invalid="ignore", over="ignore"):
        return (weights(w)[None, :, None] * d).astype(f32).reshape(-1, L * F)


def addends(p, d_out, res, T, F, L, w, levels=None):
    """(int64 flat index, float32 value) of every addend of the weighted scatter: levels with w == 0 contribute none."""
    w = weights(w)
    lv = [l for l in (range(L) if levels is None else levels) if w[l] != 0]
    return R.addends(p, premultiplied(d_out, w, L, F), res, T, F, L, levels=lv)


def schedule(start_levels, iters, n_levels, it):
    """w_l = min(1, max(0, alpha - l)), alpha = start + (L - start) min(1, it / iters): double, then float32."""
    alpha = start_levels + (n_levels - start_levels) * min(1.0, it / iters)
    return np.asarray([min(1.0, max(0.0, alpha - l)) for l in range(n_levels)], dtype=np.float64).astype(f32)
