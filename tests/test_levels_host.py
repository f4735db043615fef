"""Coarse-to-fine hash-level schedule, host side (no GPU): the schedule's values, the argument checks of the level_weights
property and of NGPTrainer(level_anneal=...), the numpy reference of the weighted encoder / scatter, and the C ABI's new symbols."""
import math
import os

import numpy as np
import pytest
import torch

from tests import _hashgrid_ref as R
from tests import _levels_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
LW_SYMBOLS = ("nerf_hashgrid_forward_lw", "nerf_ngp_encode_lw", "nerf_ngp_query_fused_lw", "nerf_hashgrid_backward_ex_lw",
              "nerf_hashgrid_backward_rays_ex_lw")


def _trainer(level_anneal, n_levels=16, it=0):
    """An NGPTrainer shell: level_weights_at needs the schedule and the level count only (no device work)."""
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer, check_level_anneal
    tr = NGPTrainer.__new__(NGPTrainer)
    tr._n_levels, tr.level_anneal, tr.it = n_levels, check_level_anneal(level_anneal, n_levels), it
    return tr


def test_schedule_values():
    tr = _trainer((4, 1000))
    # alpha = 4 + 12 it / 1000
    assert tr.level_weights_at(0) == (1.0,) * 4 + (0.0,) * 12
    want1 = [1.0] * 4 + [float(f32(0.012))] + [0.0] * 11                      # alpha = 4.012
    assert list(tr.level_weights_at(1)) == want1
    assert list(tr.level_weights_at(250)) == [1.0] * 7 + [0.0] * 9           # alpha = 7 exactly
    w999 = tr.level_weights_at(999)                                          # alpha = 15.988
    assert list(w999[:15]) == [1.0] * 15 and w999[15] == float(f32(4 + 12 * 0.999 - 15)) and 0.98 < w999[15] < 1.0
    assert tr.level_weights_at(1000) is None and tr.level_weights_at(5000) is None       # all ones: the option is off
    from nerf_meets_mlx_amd.engine.ngp import level_anneal_weights
    for it in (1000, 5000):
        assert level_anneal_weights(4, 1000, 16, it) == (1.0,) * 16
    for it in (0, 1, 250, 999, 1000, 5000):
        assert level_anneal_weights(16, 1000, 16, it) == (1.0,) * 16        # start = L: all ones at every iteration
        got = np.asarray(level_anneal_weights(4, 1000, 16, it), dtype=f32)
        assert np.array_equal(got, LR.schedule(4, 1000, 16, it))
        assert all(float(f32(v)) == v for v in level_anneal_weights(4, 1000, 16, it))     # float32-representable
    t16 = _trainer((16, 10))
    assert t16.level_weights_at(0) == (1.0,) * 16 and t16.level_weights_at(10) is None
    assert _trainer(None).level_weights_at(0) is None


def test_schedule_is_monotone_and_reaches_one():
    from nerf_meets_mlx_amd.engine.ngp import level_anneal_weights
    prev = np.zeros(16)
    for it in range(0, 41):
        w = np.asarray(level_anneal_weights(4, 40, 16, it))
        assert (w >= prev).all() and (np.diff(w) <= 0).all() and ((w >= 0) & (w <= 1)).all()
        prev = w
    assert (prev == 1).all()


def test_property_validation():
    from nerf_meets_mlx_amd.encoding.multi_hash import MultiHashEncoding, check_level_weights
    enc = MultiHashEncoding(3, 16, 16, 2048, 2, 4, device="cpu")
    assert enc.level_weights is None
    enc.level_weights = [0.5] * 16
    assert enc.level_weights == (0.5,) * 16
    enc.level_weights = np.linspace(0, 1, 16, dtype=np.float32)
    assert enc.level_weights[0] == 0.0 and enc.level_weights[-1] == 1.0
    enc.level_weights = torch.ones(16)
    assert enc.level_weights == (1.0,) * 16
    enc.level_weights = None
    assert enc.level_weights is None and enc._lw_c is None
    for bad in ([0.5] * 15, [0.5] * 17, [], [True] + [1.0] * 15, [math.nan] + [1.0] * 15, [math.inf] + [1.0] * 15,
                [-1e-6] + [1.0] * 15, [1.0 + 1e-6] + [1.0] * 15, ["a"] + [1.0] * 15, [None] + [1.0] * 15, 0.5, "0.5"):
        with pytest.raises(ValueError, match="level_weights"):
            enc.level_weights = bad
        assert enc.level_weights is None                     # a refused value leaves the property as it was
    assert check_level_weights([1] * 16, 16) == (1.0,) * 16  # integers are numbers


def test_constructor_validation():
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer, check_level_anneal
    assert check_level_anneal(None, 16) is None
    assert check_level_anneal((4, 1000), 16) == (4, 1000) and check_level_anneal([16, 1], 16) == (16, 1)
    assert check_level_anneal((1, 1), 16) == (1, 1)
    for bad in ((0, 10), (17, 10), (4, 0), (4, -1), (4.0, 10), (4, 10.0), (True, 10), (4, True), (4,), (4, 10, 1), 4, "4,10",
                (None, 10)):
        with pytest.raises(ValueError, match="level_anneal"):
            check_level_anneal(bad, 16)
        with pytest.raises(ValueError, match="level_anneal"):        # the check comes before any device work
            NGPTrainer(None, None, None, device="cpu", level_anneal=bad)
    with pytest.raises(ValueError, match="level_anneal"):            # start_levels is held to the field's level count
        NGPTrainer(None, None, None, device="cpu", level_anneal=(9, 10), n_levels=8)


@pytest.mark.parametrize("kw", [dict(bound=None), dict(occupancy_grid=False), dict(march_steps=None),
                                dict(occupancy_grid=True, march_steps=64), dict(precision=16), dict(precision=22)])
def test_level_anneal_is_accepted_in_every_mode(kw):
    """No combination of level_anneal with a mode is refused, and the trainer has taken the setting in: whatever stops a
    construction without a device, it comes behind the argument checks and is not one of them (ValueError)."""
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    tr = NGPTrainer.__new__(NGPTrainer)
    try:
        tr.__init__(torch.zeros(2, 4, 4, 3), None, None, device="cpu", level_anneal=(4, 10), **kw)
    except ValueError as e:
        pytest.fail(f"level_anneal=(4, 10) with {kw} was refused: {e}")
    except Exception:
        pass                                                 # no device here: the construction cannot finish
    assert tr.level_anneal == (4, 10)                        # consumed as the schedule, not passed on to the field
    assert tr.level_weights_at(0) == (1.0,) * 4 + (0.0,) * 12 and tr.level_weights_at(10) is None
    assert tr.march_steps == kw.get("march_steps")


def test_reference_weighted_encode_and_addends():
    rng = np.random.default_rng(3)
    L, F, T = 6, 2, 64
    res = [2, 3, 5, 8, 13, 21]
    p = rng.random((50, 3), dtype=f32)
    tables = rng.standard_normal((L, T, F)).astype(f32)
    w = np.asarray([1.0, 0.0, 0.25, 0.7, 0.0, 1.0], f32)
    base = R.encode(p, tables, res).reshape(50, L, F)
    poisoned = tables.copy()
    poisoned[w == 0] = np.nan
    got = LR.encode(p, poisoned, res, w).reshape(50, L, F)
    assert not np.isnan(got).any()
    assert np.array_equal(got[:, w == 1], base[:, w == 1])
    assert np.array_equal(got[:, 2], f32(0.25) * base[:, 2]) and np.array_equal(got[:, 3], f32(0.7) * base[:, 3])
    assert (got[:, w == 0] == 0).all() and not np.signbit(got[:, w == 0]).any()
    assert np.array_equal(LR.encode(p, tables, res, np.ones(L, f32)), R.encode(p, tables, res))
    d = rng.standard_normal((50, L * F)).astype(f32)
    idx, val = LR.addends(p, d, res, T, F, L, w)
    lv = idx // (T * F)
    assert set(np.unique(lv)) == {0, 2, 3, 5}                # masked levels have no addends at all
    i1, v1 = R.addends(p, d, res, T, F, L, levels=[0, 5])
    keep = np.isin(lv, [0, 5])
    assert np.array_equal(idx[keep], i1) and np.array_equal(val[keep], v1)
    with pytest.raises(AssertionError):
        LR.weights([0.5, 1.5])


def test_abi_declares_the_level_weight_entries():
    from nerf_meets_mlx_amd import _native
    text = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    for s in LW_SYMBOLS:
        assert f"int {s}(" in text, f"{s} is not declared in include/nerf_hip.h"
        assert "level_weights_host" in text.split(f"int {s}(")[1].split(";")[0]
        assert s in _native.SIGNATURES
        assert hasattr(_native.lib(), s), f"{s} is not exported"
        base = s[:-3] if s != "nerf_ngp_query_fused_lw" else "nerf_ngp_query_fused_h"
        assert len(_native.SIGNATURES[s][1]) == len(_native.SIGNATURES[base][1]) + 1      # the base's arguments plus w
