"""Hash-grid reference, host side (no GPU): tests/_hashgrid_ref.py against the float64 oracle, the fixed-point conversion at its
edges, the exact int64 reduction, and the inputs that exhaust the combine kernel's probe window."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import _hashgrid_ref as R


def _positions(M, seed):
    rng = np.random.default_rng(seed)
    p = rng.random((M, 3)).astype(np.float32)
    p[: M // 8] = (rng.integers(0, 17, (M // 8, 3)) / 16).astype(np.float32)         # lattice points of N = 16
    p[M // 8: M // 4] = rng.uniform(-1.5, 2.5, (M // 4 - M // 8, 3)).astype(np.float32)  # outside the unit cube
    return p


@pytest.mark.parametrize("F,L,log2_T", [(1, 3, 4), (2, 16, 12), (4, 5, 19), (8, 4, 12)])
def test_forward_emulation_agrees_with_the_float64_oracle(F, L, log2_T):
    rng = np.random.default_rng(F * 100 + L)
    T = 1 << log2_T
    res = O.hashgrid_resolutions(L, 16, 2048)
    tables = rng.standard_normal((L, T, F)).astype(np.float32)
    p = _positions(997, seed=L)
    got = R.encode(p, tables, res)
    want = O.hashgrid_encoding(torch.from_numpy(p).double(), torch.from_numpy(tables).double(), res).numpy()
    # the same float32 positions: the emulation differs from the float64 lerps by its roundings of the lerps (a few ulp of
    # max |table|) and of xs = p N_l (each offset by at most half an ulp of xs, the lerp's slope per axis at most 2 max |table|);
    # a wrong corner, weight or hash would differ by O(|table|)
    tmax = float(np.abs(tables).max())
    for l in range(L):
        ulp_xs = float(np.spacing(np.float32(np.abs(p).max() * res[l])))
        tol = (8 * float(np.finfo(np.float32).eps) + 3 * ulp_xs) * tmax
        assert np.abs(got[:, l * F:(l + 1) * F].astype(np.float64) - want[:, l * F:(l + 1) * F]).max() <= tol, l
    assert np.abs(got.astype(np.float64) - want).max() < 1e-2 * tmax


def test_sh_emulation_agrees_with_the_float64_oracle():
    rng = np.random.default_rng(1)
    d = rng.standard_normal((500, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    for deg in range(5):
        got = R.sh(d, deg)
        want = O.sh_encoding(torch.from_numpy(d).double(), deg).numpy()
        assert got.shape == want.shape == (500, (deg + 1) ** 2)
        assert np.abs(got - want).max() <= 1e-5


def test_addends_sum_to_the_forward_weights():
    """sum over the corners of one (sample, level, feature) of the addends with g = 1 is the sum of the trilinear weights
    (1 up to rounding); each addend lands in the same table row as the forward's gather of that corner."""
    rng = np.random.default_rng(2)
    L, T, F = 3, 1 << 12, 2
    res = [16, 23, 64]
    p = rng.random((100, 3)).astype(np.float32)
    idx, val = R.addends(p, np.ones((100, L * F), np.float32), res, T, F, L)
    assert idx.shape == val.shape == (100 * L * 8 * F,)
    s = val.reshape(L, 8, 100, F).astype(np.float64).sum(1)
    assert np.abs(s - 1).max() < 1e-6
    rows = idx.reshape(L, 8, 100, F)[:, :, :, 0] // F
    for l in range(L):
        c, _ = R.corners(p, res[l], T)
        assert np.array_equal(rows[l] - l * T, c.T.astype(np.int64))


def test_to_fixed_edges():
    up = np.nextafter(np.float32(256), np.float32(np.inf))
    v = np.array([256, up, -256, -up, 0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, np.nan, np.inf, -np.inf, 1.0,
                  2.0 ** -53, 3 * 2.0 ** -53, 2.0 ** -52 * 2.5], np.float32)
    q = R.to_fixed(v)
    sat = (1 << 60) + (1 << 59)
    assert q.dtype == np.int64
    assert q.tolist() == [256 << 52, sat, -(256 << 52), -sat, 0, 0, 0, 0, 0, 1 << 61, 1 << 61, 1 << 61, 1 << 52,
                          0, 2, 2]                                                  # round half to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2


def test_exact_reduction_matches_python_ints_and_wraps():
    rng = np.random.default_rng(3)
    size = 17
    idx = rng.integers(0, size, 400)
    q = rng.integers(-(1 << 62), 1 << 62, 400, dtype=np.int64)
    q[:40] = (1 << 60) + (1 << 59)                  # saturated addends on a few entries: their sum wraps mod 2^64
    idx[:40] = 5
    prefill = rng.integers(-(1 << 63), (1 << 63) - 1, size, dtype=np.int64)
    got = R.scatter_fixed(idx, q, size, prefill)
    want = [int(x) for x in prefill]
    for i, a in zip(idx.tolist(), q.tolist()):
        want[i] += a
    wrap = [((w + (1 << 63)) % (1 << 64)) - (1 << 63) for w in want]
    assert got.tolist() == wrap
    assert any(w != x for w, x in zip(want, wrap))                                   # the case really wraps


@pytest.mark.parametrize("k,finite", [(1, False), (2, False), (10, False), (11, True), (12, False), (21, True), (32, True)])
def test_saturated_multiplicities_wrap_into_the_finite_window(k, finite):
    """k saturated addends of one sign on one entry: k 1.5 2^60 mod 2^64 reads as a finite gradient for k = 11, 21, 32."""
    a = R.scatter_fixed(np.zeros(k, np.int64), R.to_fixed(np.full(k, 1e3, np.float32)), 1)
    g = R.fixed_grad(a, 1.0)[0]
    assert bool(np.isfinite(g)) == finite
    if k in (11, 21, 32):
        assert g == {11: 128.0, 21: -128.0, 32: 0.0}[k]


def test_probe_window_is_exhausted_by_the_lattice_construction():
    """F = 2 (64 samples per chunk): 64 lattice points of N = 64 with distinct keys, all homed below slot 8: whatever the
    insertion order, at least 64 - 8 - 31 of them find no slot within HC_PROBES probes."""
    T = 1 << 19
    keys, _ = R.lattice_keys(64, T)
    assert len(np.unique(keys[R.hc_slot(keys) < 8])) == 1688
    p = R.probe_lattice_points(64, T, 64, 8)
    cf, cc, off = R._cells(p, 64)
    assert np.array_equal(cf, cc) and not off.any()                                   # every corner collapses to one key
    k = R.corners(p, 64, T)[0][:, 0].astype(np.int64)
    assert len(set(k.tolist())) == 64 and (R.hc_slot(k) < 8).all()
    rng = np.random.default_rng(4)
    for order in [np.arange(64), np.arange(64)[::-1]] + [rng.permutation(64) for _ in range(20)]:
        need = R.probes_needed(k, order)
        assert sum(n > R.HC_PROBES for n in need.values()) >= 64 - 8 - 31


def test_probe_window_is_exhausted_by_the_edge_construction():
    """F = 4 (32 samples per chunk): lattice points give at most 32 keys; 32 y- / z-edges give 64 keys homed below slot 16
    (105 such edges at N = 64); x-edges hardly ever do (their keys differ in the low bits only)."""
    T = 1 << 19
    keys, ijk = R.lattice_keys(64, T)
    ok = R.hc_slot(keys) < 16
    counts = []
    for axis, stride in ((0, 1), (1, 65), (2, 65 * 65)):
        a = np.flatnonzero(ok & (ijk[:, axis] < 64))
        counts.append(int(ok[a + stride].sum()))
    assert counts[0] <= 1 and counts[1] + counts[2] == 105
    p, k = R.probe_edges(64, T, 32, 16)
    c = R.corners(p, 64, T)[0].astype(np.int64)
    assert all(set(row.tolist()) == {a, b} for row, a, b in zip(c, k[0::2], k[1::2]))   # two keys per sample
    assert len(set(k.tolist())) == 64 and (R.hc_slot(k) < 16).all()
    rng = np.random.default_rng(5)
    keys_in_order = c.reshape(-1)
    for _ in range(20):
        need = R.probes_needed(keys_in_order, rng.permutation(len(keys_in_order)))
        assert sum(n > R.HC_PROBES for n in need.values()) >= 64 - 16 - 31


def test_adam_emulation_matches_a_float64_step():
    rng = np.random.default_rng(6)
    p, g, m = (rng.standard_normal(1000).astype(np.float32) for _ in range(3))
    v = rng.random(1000).astype(np.float32)
    c1, c2 = R.bias_factors(0.9, 0.99, True, 3)
    assert abs(float(c1) - 1 / (1 - 0.9 ** 3)) < 1e-6 * float(c1)
    pn, mn, vn = R.adam_ex(p, g, m, v, 1e-2, 0.9, 0.99, 1e-8, c1, c2, 0.5)
    gd = g.astype(np.float64) * 0.5
    md = 0.9 * m + 0.1 * gd
    vd = 0.99 * v + 0.01 * gd * gd
    pd = p - 1e-2 * (md * float(c1)) / (np.sqrt(vd * float(c2)) + 1e-8)
    assert np.abs(mn - md).max() < 1e-6 and np.abs(vn - vd).max() < 1e-6 and np.abs(pn - pd).max() < 1e-6
    a = np.array([(1 << 60) - 1, -(1 << 60) + 1, 1 << 60, -(1 << 60), 1 << 61, (1 << 60) + (1 << 59)], np.int64)
    gf = R.fixed_grad(a, 1.0)
    assert np.isfinite(gf[:2]).all() and np.isnan(gf[2:]).all()
