"""The three tests every argument check of the mesh layer is built from: an integer in a range, a finite
real with optional bounds and an optional rounding to float32, and a tensor of a given dtype, shape, contiguity and device.
`is_*` answer; `need_*` refuse with ValueError(f"{noun} must be {want}, got {x!r}") and return the value normalised.  A refusal
whose text does not have that form stays with its caller, built on the `is_*` form."""
import math
import numbers

import numpy as np
import torch

F32_MAX = float(np.finfo(np.float32).max)


def is_int(x, lo=None, hi=None) -> bool:
    """x is integral, not a bool, and in [lo, hi] (None: no bound)."""
    return not isinstance(x, bool) and isinstance(x, numbers.Integral) and (lo is None or lo <= int(x)) and (hi is None or int(x) <= hi)


def need_int(x, noun, lo, hi=None, want=None) -> int:
    """int(x); `want` replaces "an int in [lo, hi]" in the text."""
    if not is_int(x, lo, hi):
        raise ValueError(f"{noun} must be {want or f'an int in [{lo}, {hi}]'}, got {x!r}")
    return int(x)


def is_number(x) -> bool:
    """x is a real number and not a bool (NaN and the infinities are)."""
    return not isinstance(x, bool) and isinstance(x, numbers.Real)


def f32(x) -> float:
    """x rounded to float32, as the library receives it; beyond float32 an infinity."""
    with np.errstate(over="ignore"):
        return float(np.float32(float(x)))


def need_real(x, noun, want="a finite number", above=None, least=None, most=None, as_f32=False) -> float:
    """float(x), not rounded; refused unless x is a finite number and v > above, v >= least and v <= most (None: no bound) for
    v = x, or with `as_f32` for v = f32(x)."""
    ok = is_number(x) and math.isfinite(float(x))
    if ok:
        v = f32(x) if as_f32 else float(x)
        ok = (above is None or v > above) and (least is None or v >= least) and (most is None or v <= most)
    if not ok:
        raise ValueError(f"{noun} must be {want}, got {x!r}")
    return float(x)


def is_tensor(t, dtype, shape=None, device=None) -> bool:
    """t is a contiguous tensor of `dtype`, of `shape` (a None entry: any size; None: any shape) and on `device` (None: any)."""
    return torch.is_tensor(t) and t.dtype == dtype \
        and (shape is None or (t.dim() == len(shape) and all(s is None or s == d for s, d in zip(shape, t.shape)))) \
        and t.is_contiguous() and (device is None or t.device == device)


def need_tensor(t, noun, dtype, shape, device=None, shown=None):
    """Refuses unless is_tensor; the text shows `shown` for the shape (default: the shape itself) and, with a device, says that
    it must be the vertices'."""
    if not is_tensor(t, dtype, shape, device):
        raise ValueError(f"{noun} must be a contiguous {str(dtype)[6:]} {shown or list(shape)} tensor"
                         + (" on the vertices' device" if device is not None else ""))
