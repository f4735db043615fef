"""Multiresolution hash grid (`mlx_nerf/encoding/multi_hash.py:13-136`), intended semantics.

The committed reference class cannot run; this follows its formulas
(growth factor :35-37, N_l :40, T :43, hash :61-77, corner / lerp order :93-131) with the
host evaluating b in float64 and the hash in uint32 wrap-around arithmetic.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import _native as N
from . import Encoding


def check_level_weights(w, n_levels: int):
    """None, or the weights as a tuple of n_levels float32-rounded Python floats in [0, 1].  ValueError for a wrong length, a
    bool, a non-number, or a non-finite or out-of-range value."""
    if w is None:
        return None
    if isinstance(w, (str, bytes)) or not hasattr(w, "__len__"):
        raise ValueError(f"level_weights: need a sequence of {n_levels} numbers in [0, 1] or None, got {w!r}")
    if torch.is_tensor(w):
        w = w.detach().cpu().tolist()
    w = list(w)
    if len(w) != n_levels:
        raise ValueError(f"level_weights: need {n_levels} values (one per level), got {len(w)}")
    out = []
    for v in w:
        if isinstance(v, (bool, np.bool_)):
            raise ValueError(f"level_weights: {v!r} is a bool, not a number")
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"level_weights: {v!r} is not a number") from None
        if not math.isfinite(v) or v < 0.0 or v > 1.0:
            raise ValueError(f"level_weights: {v!r} is not a finite value in [0, 1]")
        out.append(float(np.float32(v)))
    return tuple(out)


_CURRENT = object()           # backward(level_weights=...): "the property as it stands"


class MultiHashEncoding(Encoding):
    def __init__(self, in_dim: int, n_levels: int, min_res: int, max_res: int, n_features_per_level: int,
                 log2_hashmap_size: int, hash_init_scale: float = 0.0001, device="cuda", seed: int = 0) -> None:
        super().__init__(in_dim)
        assert in_dim == 3, "hash grid is implemented for 3-D inputs"
        self.n_levels, self.min_res, self.max_res = n_levels, min_res, max_res
        self.n_features_per_level, self.log2_hashmap_size = n_features_per_level, log2_hashmap_size
        self.growing_factor = math.exp((math.log(max_res) - math.log(min_res)) / (n_levels - 1)) if n_levels > 1 else 1.0
        self.scaled_res = [int(math.floor(min_res * self.growing_factor ** l + 1e-9)) for l in range(n_levels)]
        self.hash_table_size = 2 ** log2_hashmap_size
        g = torch.Generator(device="cpu").manual_seed(seed)
        t = (torch.rand(n_levels, self.hash_table_size, n_features_per_level, generator=g) * 2 - 1) * hash_init_scale
        self.tables = t.to(device)                                    # U(-1e-4, 1e-4): paper / intent (:51)
        self.grad = torch.zeros_like(self.tables)
        self._res_c = (C.c_int * n_levels)(*self.scaled_res)
        self._lw, self._lw_c = None, None

    @property
    def level_weights(self):
        """Per-level weights w[n_levels] in [0, 1] (a tuple) or None (the default: the `_lw` entries get NULL and run the kernels without
        weights).
        Forward: feature (l, f) = w[l] * interpolation, a level with w[l] == 0 is not read; backward: the table gradient of
        level l is that of w[l] * d_out, a level with w[l] == 0 is not touched (include/nerf_hip.h, "Level weights")."""
        return self._lw

    @level_weights.setter
    def level_weights(self, w):
        self._lw = check_level_weights(w, self.n_levels)
        self._lw_c = None if self._lw is None else (C.c_float * self.n_levels)(*self._lw)

    def get_out_dim(self):
        return self.n_levels * self.n_features_per_level

    def __call__(self, in_array: torch.Tensor):
        x = N.f32(in_array)
        out = torch.empty(x.shape[0], self.get_out_dim(), dtype=torch.float32, device=x.device)
        N.check(N.lib().nerf_hashgrid_forward_lw(N.ptr(x), x.shape[0], N.ptr(self.tables), self.n_levels,
                                                 self.log2_hashmap_size, self.n_features_per_level, self._res_c,
                                                 self._lw_c, N.ptr(out), N.stream()))       # _lw_c None: NULL, no weights
        return out

    def backward(self, in_array: torch.Tensor, d_out: torch.Tensor, level_weights=_CURRENT):
        """self.grad += d(out)/d(tables)^T d_out.  A float32 `self.grad` is accumulated with float atomics; an int64
        `self.grad` (engine/ngp.py, deterministic mode) holds 2^-52 fixed-point accumulators added with integer atomics.
        level_weights: the weights of the forward pass this is the gradient of -- None, a sequence as for the property, or
        the C array an earlier setting of the property made (HashNeRF keeps the one of its last training query); default: the
        current property."""
        x, g = N.f32(in_array), N.f32(d_out)
        if level_weights is _CURRENT:
            lw_c = self._lw_c
        elif level_weights is None or isinstance(level_weights, C.c_float * self.n_levels):
            lw_c = level_weights
        else:
            lw_c = (C.c_float * self.n_levels)(*check_level_weights(level_weights, self.n_levels))
        N.check(N.lib().nerf_hashgrid_backward_ex_lw(N.ptr(x), x.shape[0], N.ptr(g), self.n_levels, self.log2_hashmap_size,
                                                     self.n_features_per_level, self._res_c, lw_c, 0, self.n_levels,
                                                     int(self.grad.dtype == torch.int64), N.ptr(self.grad), N.stream()))
        return self.grad
