"""Hash-grid encoder, table-gradient scatter and the Adam steps that consume it (csrc/encode.hip, csrc/adam.hip) on the GPU, against
the float32 emulation of tests/_hashgrid_ref.py.

The library is built with -ffp-contract=off and keeps f32 subnormals, and every operation of these kernels is one IEEE float32
add, multiply, floor, ceil, division or square root: the forward features, SH columns and sample positions must match the
emulation BIT FOR BIT.  Fixed-point addition is associative: the deterministic accumulators must equal the host's int64 sum of
the quantised addends bit for bit, whatever the path (direct / LDS write-combining / probe fallback), level grouping or
schedule.  The float-atomic scatter is held to the summation bound (k + 1) 2^-24 (sum |a| + |prefill|) per entry.

The C entry points are called through _native, so that F, L, log2_T, level ranges and "hash_combine_max_res" can be chosen
freely; every output is filled with a sentinel first."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from nerf_meets_mlx_amd import _native as N
from oracle import nerf_oracle as O
from tests import _hashgrid_ref as R
from tests._poison import SENTINEL, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
ENGINE_RES = O.hashgrid_resolutions(16, 16, 2048)
BOUND_SCALE, BOUND_OFFSET = 1.0 / (2.0 * 1.5), 0.5          # HashNeRF(bound=1.5): the scene box onto the unit cube
NPOT = [3, 5, 7, 11, 13, 17, 23, 30, 37, 61, 64, 99, 127, 255, 1000, 2047]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _ires(res):
    return (C.c_int * len(res))(*[int(r) for r in res])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@contextlib.contextmanager
def _combine(max_res):
    lib = N.lib()
    old = lib.nerf_get_option(b"hash_combine_max_res")
    N.check(lib.nerf_set_option(b"hash_combine_max_res", int(max_res)))
    try:
        yield
    finally:
        N.check(lib.nerf_set_option(b"hash_combine_max_res", old))


def _res_list(kind, L, seed):
    rng = np.random.default_rng(seed)
    if kind == "engine":
        return O.hashgrid_resolutions(L, 16, 2048)
    if kind == "npot":
        return sorted(rng.choice(NPOT, L).tolist())
    return rng.choice(NPOT + [16, 32, 512, 2048], L).tolist()          # "mixed": non-monotone


def _roundup_coords(res):
    """float32 p with float32(p N) an integer while p N (exact) is not: the rounding decides the cell."""
    out = []
    for r in sorted(set(int(x) for x in res)):
        k = np.arange(1, r)
        base = (k / r).astype(f32)
        for p in (base, np.nextafter(base, f32(2)), np.nextafter(base, f32(-1))):
            xs = p * f32(r)
            exact = p.astype(np.float64) * r
            out.append(p[(xs == np.floor(xs)) & (exact != np.floor(exact))])
    return np.concatenate(out) if out else np.zeros(0, f32)


def _positions(M, res, seed, nan=False):
    """[M, 3] float32: uniform in the unit cube mixed per coordinate with lattice points, 0 / 1 / nextafter(1, 0), coordinates
    outside [0, 1] (int32 -> uint32 wrap of negative cells in the hash), and float32 round-up cases; NaN rows on request."""
    rng = np.random.default_rng(seed)
    p = rng.random((M, 3), dtype=f32)
    kind = rng.integers(0, 8, (M, 3))
    lat = (rng.integers(0, 2049, (M, 3)) // rng.choice([1, 4, 128], (M, 3))).astype(np.float64)
    den = rng.choice([16.0, 64.0, 2048.0], (M, 3))
    p = np.where(kind == 1, (np.minimum(lat, den) / den).astype(f32), p)
    special = np.array([0.0, 1.0, np.nextafter(f32(1), f32(0))], f32)
    p = np.where(kind == 2, special[rng.integers(0, 3, (M, 3))], p)
    outside = np.where(rng.random((M, 3)) < 0.5, rng.uniform(-1.5, 0, (M, 3)), rng.uniform(1, 2.5, (M, 3))).astype(f32)
    p = np.where(kind == 3, outside, p)
    ru = _roundup_coords(res)
    if len(ru):
        p = np.where(kind == 4, ru[rng.integers(0, len(ru), (M, 3))], p)
    if nan:
        rows = rng.random(M) < 0.03
        p[rows, rng.integers(0, 3, int(rows.sum()))] = np.nan
    return np.ascontiguousarray(p, dtype=f32)


def _rays(B, seed):
    """rays [B, 11] (o in the [-1.5, 1.5] box and a little beyond, unit d, view direction = d), z [B, n] sorted depths."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.8, 1.8, (B, 3))
    d = rng.standard_normal((B, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((B, 1), 2.0), np.full((B, 1), 6.0), d], 1).astype(f32)
    return rays


# ------------------------------------------------------------------------------------------------------------------ forward
FWD_CASES = [  # F, L, log2_T, M, resolutions
    (1, 1, 1, 1, "engine"), (1, 5, 12, 1000, "mixed"), (1, 32, 19, 1000, "npot"), (1, 4, 4, 64, "engine"),
    (2, 16, 19, 1000, "engine"), (2, 3, 4, 63, "npot"), (2, 32, 12, 65, "mixed"),
    (4, 4, 12, 64, "npot"), (4, 32, 12, 65, "engine"), (4, 5, 1, 1000, "mixed"),
    (8, 5, 19, 1000, "mixed"), (8, 16, 4, 1000, "npot"), (8, 1, 12, 63, "engine"), (8, 3, 12, 1, "npot"),
]


def _forward(p, tables, res, F, L, log2_T):
    M = p.shape[0]
    out = sentinel_(torch.empty(M, L * F, dtype=torch.float32, device=DEV))
    pd, td = _dev(p), _dev(tables)          # held until the launch: a freed block would be handed to the next allocation
    N.check(N.lib().nerf_hashgrid_forward(N.ptr(pd), M, N.ptr(td), L, log2_T, F, _ires(res), N.ptr(out), N.stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("F,L,log2_T,M,kind", FWD_CASES)
def test_forward_is_bit_exact(F, L, log2_T, M, kind):
    seed = F * 1000 + L * 10 + log2_T
    res = _res_list(kind, L, seed)
    rng = np.random.default_rng(seed)
    tables = rng.standard_normal((L, 1 << log2_T, F)).astype(f32)
    p = _positions(M, res, seed, nan=M > 1)
    out = _forward(p, tables, res, F, L, log2_T)
    assert unwritten(out) == 0
    got = _host(out)
    want = R.encode(p, tables, res)
    nan_rows = np.isnan(p).any(1)
    assert np.isnan(got[nan_rows]).all()                                   # a NaN position: every feature of its row NaN
    bad = np.flatnonzero((_bits(got[~nan_rows]) != _bits(want[~nan_rows])).any(1))
    assert len(bad) == 0, (len(bad), p[~nan_rows][bad[:4]], got[~nan_rows][bad[:1]], want[~nan_rows][bad[:1]])


def test_forward_grid_stride_loop_is_bit_exact():
    """M > 256 x 256 x 32: each thread of the forward serves more than one sample."""
    M, F, L, log2_T = 2_200_000, 2, 1, 19
    rng = np.random.default_rng(7)
    tables = rng.standard_normal((L, 1 << log2_T, F)).astype(f32)
    res = [ENGINE_RES[-1]]
    p = _positions(M, res, 7)
    out = _forward(p, tables, res, F, L, log2_T)
    assert unwritten(out) == 0
    assert np.array_equal(_bits(_host(out)), _bits(R.encode(p, tables, res)))


# --------------------------------------------------------------------------------------------------------- nerf_ngp_encode
NGP_CASES = [  # B, n, F, L, log2_T, sh_degree, bound, pts_out
    (3, 1, 2, 16, 19, 4, True, True), (5, 7, 1, 5, 12, 0, False, False), (2, 64, 4, 3, 12, 1, True, True),
    (37, 192, 8, 4, 12, 2, True, False), (11, 64, 2, 16, 19, 3, False, True), (1, 7, 2, 32, 4, 4, True, False),
]


@pytest.mark.parametrize("B,n,F,L,log2_T,deg,bound,with_pts", NGP_CASES)
def test_ngp_encode_rows_are_bit_exact(B, n, F, L, log2_T, deg, bound, with_pts):
    seed = B * 7 + n
    rng = np.random.default_rng(seed)
    res = O.hashgrid_resolutions(L, 16, 2048) if L == 16 else _res_list("mixed", L, seed)
    tables = rng.standard_normal((L, 1 << log2_T, F)).astype(f32)
    rays = _rays(B, seed)
    z = np.sort(rng.uniform(0, 4, (B, n)), 1).astype(f32)
    scale, offset = (BOUND_SCALE, BOUND_OFFSET) if bound else (1.0, 0.0)
    M, stride = B * n, L * F + (deg + 1) ** 2
    x_out = sentinel_(torch.empty(M, stride, dtype=torch.float32, device=DEV))
    pts = sentinel_(torch.empty(M, 3, dtype=torch.float32, device=DEV)) if with_pts else None
    rd, zd, td = _dev(rays), _dev(z), _dev(tables)
    N.check(N.lib().nerf_ngp_encode(N.ptr(rd), N.ptr(zd), B, n, N.ptr(td), L, log2_T, F, _ires(res), deg, scale, offset,
                                    N.ptr(x_out), N.ptr(pts), N.stream()))
    assert unwritten(x_out) == 0
    got = _host(x_out)
    p = R.points(rays, z, n, scale, offset)
    assert np.array_equal(_bits(got[:, :L * F]), _bits(R.encode(p, tables, res)))
    assert np.array_equal(_bits(got[:, L * F:]), _bits(R.sh(rays[np.arange(M) // n, 8:11], deg)))
    if with_pts:
        assert unwritten(pts) == 0
        assert np.array_equal(_bits(_host(pts)), _bits(p))


# --------------------------------------------------------------------------------------------------------- table gradient
def _bwd(p, d_out, L, log2_T, F, res, lo, hi, fixed, acc):
    N.check(N.lib().nerf_hashgrid_backward_ex(N.ptr(p), p.shape[0], N.ptr(d_out), L, log2_T, F, _ires(res), lo, hi, int(fixed),
                                              N.ptr(acc), N.stream()))


def _prefill(size, fixed, seed):
    rng = np.random.default_rng(seed)
    if fixed:
        return rng.integers(-(1 << 62), 1 << 62, size, dtype=np.int64)
    return (rng.standard_normal(size) * 1e-2).astype(f32)


def _scatter(p, d_out, L, log2_T, F, res, fixed, prefill, lo=0, hi=None, combine=64):
    """The accumulator [L T F] after one nerf_hashgrid_backward_ex over levels [lo, hi) (host arrays in, host array out)."""
    acc = _dev(prefill)
    with _combine(combine):
        _bwd(_dev(p), _dev(d_out), L, log2_T, F, res, lo, L if hi is None else hi, fixed, acc)
        return _host(acc)


def _want_fixed(p, d_out, L, log2_T, F, res, prefill, levels=None):
    idx, val = R.addends(p, d_out, res, 1 << log2_T, F, L, levels)
    return R.scatter_fixed(idx, R.to_fixed(val), prefill.size, prefill)


def _check_float(got, prefill, p, d_out, L, log2_T, F, res, levels=None):
    """Per entry |got - prefill - exact| <= (k + 1) 2^-24 (sum |a| + |prefill|) (+ k 2^-126 for subnormals); an entry with a
    non-finite addend is non-finite."""
    idx, val = R.addends(p, d_out, res, 1 << log2_T, F, L, levels)
    fin = np.isfinite(val)
    s, sa, k = R.scatter_f64(idx[fin], val[fin], prefill.size)
    poisoned = np.bincount(idx[~fin], minlength=prefill.size) > 0
    assert not np.isfinite(got[poisoned]).any()
    ok = ~poisoned
    pre = prefill.astype(np.float64)
    err = np.abs(got[ok].astype(np.float64) - pre[ok] - s[ok])
    bound = (k[ok] + 1) * 2.0 ** -24 * (sa[ok] + np.abs(pre[ok])) + k[ok] * 2.0 ** -126
    bad = np.flatnonzero(err > bound)
    assert len(bad) == 0, (len(bad), err[bad[:4]], bound[bad[:4]], k[ok][bad[:4]])


SCATTER_RES = [16, 24, 30, 40, 64, 181, 33, 2048]            # "30" splits the combined leading levels mid-way; 33 after 181: direct
PATHS = [(1, 0), (2, 0), (4, 0), (8, 0), (2, 64), (2, 30), (4, 64), (4, 30)]   # (F, hash_combine_max_res)


def _grads(M, L, F, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((M, L * F)).astype(f32)
    g[rng.random(g.shape) < 0.05] = 0.0
    g[rng.random(g.shape) < 0.02] *= f32(2.0 ** -30)            # small addends: a dropped one shows in fixed point
    return g


@pytest.mark.parametrize("F,combine", PATHS)
@pytest.mark.parametrize("log2_T", [12, 19])
def test_fixed_scatter_is_bit_exact(F, combine, log2_T):
    L, M = len(SCATTER_RES), 1000
    p = _positions(M, SCATTER_RES, 11 + F)
    d_out = _grads(M, L, F, 12 + F)
    prefill = _prefill(L * (1 << log2_T) * F, True, 13)
    got = _scatter(p, d_out, L, log2_T, F, SCATTER_RES, True, prefill, combine=combine)
    want = _want_fixed(p, d_out, L, log2_T, F, SCATTER_RES, prefill)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("F,combine", PATHS)
def test_float_scatter_is_within_the_summation_bound(F, combine):
    L, M, log2_T = len(SCATTER_RES), 1000, 12
    p = _positions(M, SCATTER_RES, 21 + F)
    d_out = _grads(M, L, F, 22 + F)
    prefill = _prefill(L * (1 << log2_T) * F, False, 23)
    got = _scatter(p, d_out, L, log2_T, F, SCATTER_RES, False, prefill, combine=combine)
    _check_float(got, prefill, p, d_out, L, log2_T, F, SCATTER_RES)


@pytest.mark.parametrize("F", [1, 2, 4, 8])
def test_level_ranges_touch_only_their_levels_and_sum_to_the_whole(F):
    L, M, log2_T = 9, 700, 10
    res = [16, 20, 28, 40, 64, 90, 128, 300, 2048]
    T = 1 << log2_T
    p = _positions(M, res, 31)
    d_out = _grads(M, L, F, 32)
    prefill = _prefill(L * T * F, True, 33)
    acc = _dev(prefill)
    pd, gd = _dev(p), _dev(d_out)
    for lo, hi in [(0, 1), (1, 4), (4, 9)]:
        one = _scatter(p, d_out, L, log2_T, F, res, True, prefill, lo, hi)
        want = _want_fixed(p, d_out, L, log2_T, F, res, prefill, range(lo, hi))
        assert np.array_equal(one, want), (lo, hi)
        outside = np.ones(L, bool)
        outside[lo:hi] = False
        assert np.array_equal(one.reshape(L, -1)[outside], prefill.reshape(L, -1)[outside])
        _bwd(pd, gd, L, log2_T, F, res, lo, hi, True, acc)                 # the pieces one after the other, into one buffer
    assert np.array_equal(_host(acc), _want_fixed(p, d_out, L, log2_T, F, res, prefill))


@pytest.mark.parametrize("F", [2, 4, 8])
def test_rays_entry_points_match_the_point_list(F):
    B, n, L, log2_T = 13, 64, 16, 14
    res = ENGINE_RES
    rng = np.random.default_rng(41)
    rays = _rays(B, 41)
    z = np.sort(rng.uniform(0, 4, (B, n)), 1).astype(f32)
    p = R.points(rays, z, n, BOUND_SCALE, BOUND_OFFSET)
    d_out = _grads(B * n, L, F, 42)
    rd, zd, gd = _dev(rays), _dev(z), _dev(d_out)
    size = L * (1 << log2_T) * F
    for fixed in (True, False):
        prefill = _prefill(size, fixed, 43)
        for lo, hi in [(0, L), (3, 11)]:
            acc = _dev(prefill)
            N.check(N.lib().nerf_hashgrid_backward_rays_ex(N.ptr(rd), N.ptr(zd), B, n, N.ptr(gd), L, log2_T, F, _ires(res),
                                                           BOUND_SCALE, BOUND_OFFSET, lo, hi, int(fixed), N.ptr(acc), N.stream()))
            got = _host(acc)
            if fixed:
                assert np.array_equal(got, _want_fixed(p, d_out, L, log2_T, F, res, prefill, range(lo, hi)))
                assert np.array_equal(got, _scatter(p, d_out, L, log2_T, F, res, True, prefill, lo, hi))
            else:
                _check_float(got, prefill, p, d_out, L, log2_T, F, res, range(lo, hi))
    # the float-only entry points of the same scatter
    prefill = _prefill(size, False, 44)
    acc = _dev(prefill)
    N.check(N.lib().nerf_hashgrid_backward_rays(N.ptr(rd), N.ptr(zd), B, n, N.ptr(gd), L, log2_T, F, _ires(res), BOUND_SCALE,
                                                BOUND_OFFSET, N.ptr(acc), N.stream()))
    _check_float(_host(acc), prefill, p, d_out, L, log2_T, F, res)
    acc, pd = _dev(prefill), _dev(p)
    N.check(N.lib().nerf_hashgrid_backward(N.ptr(pd), B * n, N.ptr(gd), L, log2_T, F, _ires(res), N.ptr(acc), N.stream()))
    _check_float(_host(acc), prefill, p, d_out, L, log2_T, F, res)


@pytest.mark.parametrize("F,M", [(2, 600_000), (4, 280_000)])
def test_multi_chunk_and_grid_stride_scatter_is_bit_exact(F, M):
    """Level 0 through the LDS table with more chunks than workgroups (each workgroup reuses its table and list counters: a key or
    value left over from an earlier chunk shows), level 1 direct with more (sample, feature, x-side) lanes than threads."""
    L, log2_T = 2, 19
    res = [24, 2048]
    p = _positions(M, res, 51)
    d_out = _grads(M, L, F, 52)
    prefill = _prefill(L * (1 << log2_T) * F, True, 53)
    want = _want_fixed(p, d_out, L, log2_T, F, res, prefill)
    for combine in (64, 0):
        got = _scatter(p, d_out, L, log2_T, F, res, True, prefill, combine=combine)
        assert np.array_equal(got, want), (combine, int((got != want).sum()))
    pf = _prefill(L * (1 << log2_T) * F, False, 54)
    _check_float(_scatter(p, d_out, L, log2_T, F, res, False, pf), pf, p, d_out, L, log2_T, F, res)


def test_sum_of_weights_with_looping_combine_workgroups():
    """d_out = 1: each sample spreads a total weight of 1 (up to rounding) over each level; 140 000 samples through the LDS table
    with more chunks than workgroups."""
    M, L, F, log2_T = 140_000, 2, 2, 12
    res = [16, 64]
    p = np.random.default_rng(61).random((M, 3), dtype=f32)
    d_out = np.ones((M, L * F), f32)
    prefill = np.zeros(L * (1 << log2_T) * F, f32)
    got = _scatter(p, d_out, L, log2_T, F, res, False, prefill)
    _check_float(got, prefill, p, d_out, L, log2_T, F, res)
    tot = got.reshape(L, -1, F).astype(np.float64).sum(1)
    assert np.abs(tot / M - 1).max() < 1e-5


def _probe_input(F, M, seed):
    """M samples at N = 64 (one level), the construction that exhausts the probe window in chunk 0 and in chunk 2048 (the second
    chunk of workgroup 0: the launch has 2048 workgroups)."""
    T = 1 << 19
    if F == 2:
        block = R.probe_lattice_points(64, T, 64, 8)
    else:
        block = R.probe_edges(64, T, 32, 16)[0]
    spw = 256 // (2 * F)
    p = np.random.default_rng(seed).random((M, 3), dtype=f32)
    p[:spw] = block
    p[2048 * spw:2049 * spw] = block[::-1]
    return p


@pytest.mark.parametrize("F,M", [(2, 64 * 2056), (4, 32 * 4100)])
def test_probe_exhaustion_fallback_is_exact(F, M):
    L, log2_T, res = 1, 19, [64]
    p = _probe_input(F, M, 71)
    d_out = _grads(M, L, F, 72)
    size = (1 << log2_T) * F
    for fixed in (True, False):
        prefill = _prefill(size, fixed, 73)
        got = _scatter(p, d_out, L, log2_T, F, res, fixed, prefill, combine=64)
        if fixed:
            want = _want_fixed(p, d_out, L, log2_T, F, res, prefill)
            assert np.array_equal(got, want), int((got != want).sum())
        else:
            _check_float(got, prefill, p, d_out, L, log2_T, F, res)


def _poison_input(F, seed):
    """Upstream gradients that saturate (|addend| > 256) or are NaN / Inf.  k samples on one lattice point of N = 64 each give
    that entry one addend g (the other 7 corner weights are 0): k saturated addends of one sign, k in {1, 2, 10, 11, 12, 21, 32};
    a NaN g on a lattice point gives its one entry 8 NaN addends (8 x 2^61 = 0 mod 2^64), elsewhere 8 entries one each.
    Returns positions, d_out and the (lattice point, k) of each saturated group."""
    rng = np.random.default_rng(seed)
    lat = rng.permutation(64 ** 3)[:64]
    cell = lambda j: np.array([lat[j] % 64, lat[j] // 64 % 64, lat[j] // 4096], np.float64) / 64   # noqa: E731
    p, g, groups = [], [], []
    for j, (k, sign) in enumerate([(1, 1), (2, -1), (10, 1), (11, 1), (12, -1), (21, 1), (21, -1), (32, 1), (32, -1)]):
        p += [cell(j)] * k
        g += [np.concatenate([[sign * 1e3], rng.standard_normal(F - 1)])] * k
        groups.append((cell(j), k))
    for j, v in enumerate([np.nan, np.inf, -np.inf, np.nan]):            # non-finite g on a lattice point and off the lattice
        p += [cell(20 + j), rng.random(3)]
        g += [np.full(F, v)] * 2
    p += list(rng.random((300, 3)))
    g += list(rng.standard_normal((300, F)) * 300)                        # a few saturated addends among ordinary ones
    return np.asarray(p, f32), np.asarray(g, f32).reshape(-1, F), groups


@pytest.mark.parametrize("F,combine", PATHS)
def test_saturated_and_nonfinite_addends_are_pinned(F, combine):
    L, log2_T, res = 1, 19, [64]
    p, d_out, groups = _poison_input(F, 81)
    size = (1 << log2_T) * F
    prefill = np.zeros(size, np.int64)
    got = _scatter(p, d_out, L, log2_T, F, res, True, prefill, combine=combine)
    want = _want_fixed(p, d_out, L, log2_T, F, res, prefill)
    assert np.array_equal(got, want), int((got != want).sum())
    # the window of hash_common.h: k saturated addends of one sign on an entry read as a finite gradient for k = 11, 21, 32
    g = R.fixed_grad(got, 1.0)
    for c, k in groups:
        entry = int(R.corners(c[None].astype(f32), 64, 1 << log2_T)[0][0, 0]) * F
        assert bool(np.isfinite(g[entry])) == (k in (11, 21, 32)), k
    fp = _prefill(size, False, 82)
    _check_float(_scatter(p, d_out, L, log2_T, F, res, False, fp, combine=combine), fp, p, d_out, L, log2_T, F, res)


# --------------------------------------------------------------------------------------------------------------------- Adam
LR, B1, B2, EPS = 1e-2, 0.9, 0.99, 1e-8
TAIL = 64
FIXED_EDGES = [(1 << 60) - 1, -(1 << 60) + 1, 1 << 60, -(1 << 60), 1 << 61, (1 << 60) + (1 << 59), -((1 << 60) + (1 << 59)),
               0, 1, -1, 1 << 52, (1 << 59) + 12345]


def _adam_inputs(count, fixed, seed):
    rng = np.random.default_rng(seed)
    n = count + TAIL
    p = rng.standard_normal(n).astype(f32)
    m = (rng.standard_normal(n) * 1e-2).astype(f32)
    v = (rng.random(n) * 1e-3).astype(f32)
    v[::7] = 0
    if fixed:
        g = R.to_fixed((rng.standard_normal(n) * 4).astype(f32))
        e = np.asarray(FIXED_EDGES, np.int64)[: count]
        g[: len(e)] = e
        g[count:] = np.int64(0x5A5A5A5A5A5A5A5A)
    else:
        g = (rng.standard_normal(n) * 4).astype(f32)
        g[: min(count, 4)] = np.array([0.0, -0.0, 1e-40, np.nan], f32)[: min(count, 4)]
        g[count:] = np.array([SENTINEL], np.int32).view(f32)[0]
    return p, g, m, v


def _adam_check(count, fixed, zero, shadow, bias, gscale, entry):
    p, g, m, v = _adam_inputs(count, fixed, count + 2 * fixed + zero)
    pd, gd, md, vd = _dev(p), _dev(g), _dev(m), _dev(v)
    ph = torch.full((count + TAIL,), 0x7E5A, dtype=torch.int16, device=DEV) if shadow else None
    step = 7
    lib = N.lib()
    if entry == "plain":
        N.check(lib.nerf_adam_step(N.ptr(pd), N.ptr(gd), N.ptr(md), N.ptr(vd), count, LR, B1, B2, EPS, bias, step, gscale,
                                   N.stream()))
    elif entry == "ex":
        N.check(lib.nerf_adam_step_ex(N.ptr(pd), N.ptr(gd), N.ptr(md), N.ptr(vd), count, LR, B1, B2, EPS, bias, step, gscale,
                                      int(fixed), int(zero), N.stream()))
    else:
        N.check(lib.nerf_adam_step_shadow(N.ptr(pd), N.ptr(gd), N.ptr(md), N.ptr(vd), count, LR, B1, B2, EPS, bias, step,
                                          gscale, int(fixed), int(zero), N.ptr(ph), N.stream()))
    c1, c2 = R.bias_factors(B1, B2, bias, step)
    wp, wm, wv = R.adam_ex(p[:count], g[:count], m[:count], v[:count], LR, B1, B2, EPS, c1, c2, gscale, fixed)
    gp, gg, gm, gv = _host(pd), _host(gd), _host(md), _host(vd)
    for name, got, want, full in [("p", gp, wp, p), ("m", gm, wm, m), ("v", gv, wv, v)]:
        bad = np.flatnonzero(_bits(got[:count]) != _bits(want))
        nan_ok = np.isnan(got[:count][bad]) & np.isnan(want[bad])        # a NaN's payload is not part of the contract
        assert nan_ok.all(), (name, bad[~nan_ok][:4], got[:count][bad[~nan_ok][:4]], want[bad[~nan_ok][:4]])
        assert np.array_equal(_bits(got[count:]), _bits(full[count:])), name       # nothing past count
    if zero:
        assert not gg[:count].any() and not np.signbit(gg[:count]).any()
    else:
        assert np.array_equal(gg[:count].view(np.uint8), g[:count].view(np.uint8))
    assert np.array_equal(gg[count:].view(np.uint8), g[count:].view(np.uint8))
    if shadow:
        h = ph.cpu()
        want_h = torch.from_numpy(gp[:count]).half()
        nan = torch.isnan(want_h)
        assert torch.equal(h[:count][~nan], want_h.view(torch.int16)[~nan])
        assert torch.isnan(h[:count].view(torch.float16)[nan]).all()
        assert (h[count:] == 0x7E5A).all()


@pytest.mark.parametrize("count", [1, 255, 257, 600_001])
@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("shadow", [False, True])
def test_adam_ex_variants_are_bit_exact(count, fixed, zero, shadow):
    bias, gscale = (1, 1.0 / 1024) if (count + zero) % 2 else (0, 1.0)
    _adam_check(count, fixed, zero, shadow, bias, gscale, "shadow" if shadow else "ex")
    if not shadow:
        _adam_check(count, fixed, zero, True, 1 - bias, 0.5, "shadow")


@pytest.mark.parametrize("count", [1, 257, 600_001])
@pytest.mark.parametrize("bias", [0, 1])
def test_adam_plain_is_bit_exact(count, bias):
    _adam_check(count, False, False, False, bias, 0.25 if bias else 1.0, "plain")


def test_adam_reads_saturated_multiplicities_as_the_window_says():
    """k saturated addends of one sign: finite for k = 11, 21, 32 (the documented bound in hash_common.h), NaN for k = 1, 12."""
    sat = (1 << 60) + (1 << 59)
    acc = np.array([(k * sat + (1 << 63)) % (1 << 64) - (1 << 63) for k in (1, 11, 12, 21, 32)], np.int64)
    p = np.zeros(5, f32)
    pd, gd, md, vd = _dev(p), _dev(acc), _dev(np.zeros(5, f32)), _dev(np.zeros(5, f32))
    N.check(N.lib().nerf_adam_step_ex(N.ptr(pd), N.ptr(gd), N.ptr(md), N.ptr(vd), 5, LR, B1, B2, EPS, 1, 1, 1.0, 1, 1, N.stream()))
    got = _host(pd)
    assert np.isnan(got[[0, 2]]).all() and np.isfinite(got[[1, 3, 4]]).all()
    assert got[1] < 0 < got[3] and got[4] == 0                                   # +128 and -128 gradients, 0
    want = R.adam_ex(p, acc, np.zeros(5, f32), np.zeros(5, f32), LR, B1, B2, EPS, *R.bias_factors(B1, B2, 1, 1), 1.0, True)[0]
    assert np.array_equal(_bits(got[[1, 3, 4]]), _bits(want[[1, 3, 4]])) and np.isnan(want[[0, 2]]).all()


# ------------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_and_empty_launches():
    lib, s = N.lib(), N.stream()
    E_NULL, E_SHAPE, E_UNSUP = -1, -2, -3
    res = _ires([16] * 33)
    x = _dev(np.random.default_rng(1).random((8, 3), dtype=f32))
    tables = _dev(np.ones((4, 16, 8), f32))
    out = sentinel_(torch.empty(8 * 64, dtype=torch.float32, device=DEV))
    acc = _dev(np.arange(4 * 16 * 8, dtype=np.int64))
    d_out = _dev(np.ones((8, 64), f32))
    X, T, O_, A, G = N.ptr(x), N.ptr(tables), N.ptr(out), N.ptr(acc), N.ptr(d_out)
    fwd = lambda M, L, lg, F, xx=X, tt=T, oo=O_: lib.nerf_hashgrid_forward(xx, M, tt, L, lg, F, res, oo, s)   # noqa: E731
    bwd = lambda M, L, lg, F, lo, hi, fx=1, xx=X, aa=A: lib.nerf_hashgrid_backward_ex(xx, M, G, L, lg, F, res, lo, hi, fx, aa, s)  # noqa: E731,E501
    assert fwd(8, 4, 4, 3) == E_UNSUP and bwd(8, 4, 4, 3, 0, 4) == E_UNSUP
    for L, lg in [(0, 4), (33, 4), (4, 0), (4, 31)]:
        assert fwd(8, L, lg, 2) == E_SHAPE and bwd(8, L, lg, 2, 0, max(L, 0)) == E_SHAPE
    for lo, hi in [(-1, 2), (3, 2), (0, 5)]:
        assert bwd(8, 4, 4, 2, lo, hi) == E_SHAPE
    assert bwd(8, 4, 4, 2, 0, 4, fx=2) == E_UNSUP
    assert fwd(8, 4, 4, 2, xx=None) == E_NULL and fwd(8, 4, 4, 2, tt=None) == E_NULL and fwd(8, 4, 4, 2, oo=None) == E_NULL
    assert bwd(8, 4, 4, 2, 0, 4, xx=None) == E_NULL and bwd(8, 4, 4, 2, 0, 4, aa=None) == E_NULL
    assert lib.nerf_hashgrid_forward(X, 8, T, 4, 4, 2, None, O_, s) == E_NULL
    rays = _dev(_rays(2, 3))
    z = _dev(np.ones((2, 4), f32))
    Rp, Z = N.ptr(rays), N.ptr(z)
    assert lib.nerf_ngp_encode(Rp, Z, 2, 4, T, 4, 4, 2, res, 5, 1.0, 0.0, O_, None, s) == E_SHAPE
    assert lib.nerf_ngp_encode(Rp, Z, 2, 4, T, 4, 4, 2, res, 2, 1.0, 0.0, None, None, s) == E_NULL
    assert lib.nerf_ngp_encode(Rp, Z, 2, 4, T, 4, 4, 3, res, 2, 1.0, 0.0, O_, None, s) == E_UNSUP
    assert lib.nerf_hashgrid_backward_rays_ex(Rp, None, 2, 4, G, 4, 4, 2, res, 1.0, 0.0, 0, 4, 1, A, s) == E_NULL
    assert lib.nerf_hashgrid_backward_rays_ex(Rp, Z, 2, 4, G, 4, 4, 2, res, 1.0, 0.0, 0, 4, 3, A, s) == E_UNSUP
    assert lib.nerf_hashgrid_backward_rays(Rp, Z, 2, 4, G, 4, 4, 2, res, 1.0, 0.0, None, s) == E_NULL
    p1, m1 = _dev(np.zeros(4, f32)), _dev(np.zeros(4, f32))
    assert lib.nerf_adam_step_ex(N.ptr(p1), A, N.ptr(m1), N.ptr(m1), 0, LR, B1, B2, EPS, 0, 1, 1.0, 1, 1, s) == E_SHAPE
    assert lib.nerf_adam_step_ex(N.ptr(p1), None, N.ptr(m1), N.ptr(m1), 4, LR, B1, B2, EPS, 0, 1, 1.0, 1, 1, s) == E_NULL
    assert lib.nerf_adam_step(N.ptr(p1), N.ptr(m1), N.ptr(m1), N.ptr(m1), 4, LR, B1, B2, EPS, 1, 0, 1.0, s) == E_SHAPE
    # empty launches succeed and write nothing
    out0, acc0 = out.clone(), acc.clone()
    assert fwd(0, 4, 4, 2) == 0 and bwd(0, 4, 4, 2, 0, 4) == 0 and bwd(8, 4, 4, 2, 2, 2) == 0
    assert lib.nerf_ngp_encode(Rp, Z, 0, 4, T, 4, 4, 2, res, 2, 1.0, 0.0, O_, None, s) == 0
    assert lib.nerf_ngp_encode(Rp, Z, 2, 0, T, 4, 4, 2, res, 2, 1.0, 0.0, O_, None, s) == 0
    assert lib.nerf_hashgrid_backward_rays_ex(Rp, Z, 0, 4, G, 4, 4, 2, res, 1.0, 0.0, 0, 4, 1, A, s) == 0
    assert lib.nerf_hashgrid_backward_rays_ex(Rp, Z, 2, 0, G, 4, 4, 2, res, 1.0, 0.0, 0, 4, 1, A, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), out0.view(torch.int32)) and torch.equal(acc, acc0)
