"""Level weights of the hash grid (coarse-to-fine training) on the GPU: the `_lw` entries against
tests/_levels_ref.py and against today's entries, HashNeRF's level_weights property on every query path, and
NGPTrainer(level_anneal=...).

Every comparison is bit-exact.  The stand-alone encoders are held to the float32 emulation times one float32 multiply.  The fused
query is held to the EXISTING query on tables whose level l was multiplied by w[l] in {0, 0.25, 0.5, 1}: a power-of-two scale
commutes with every rounding of the interpolation while nothing is subnormal (table magnitudes in [2^-8, 1]).  The weighted
scatter is held to the existing entry fed d_out pre-multiplied per level column by w[l] in float32 -- the operation order the
header states.  L = 16, F = 2, resolutions 16 ... 2048: the first five levels (N_l <= 64) take the LDS write-combining path.
Section 9 holds every entry without the suffix to its `_lw` entry called with NULL weights, results and error texts."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from nerf_meets_mlx_amd import _native as N
from oracle import nerf_oracle as O
from tests import _hashgrid_ref as R
from tests import _levels_ref as LR
from tests._poison import NAN_BYTES, bits_equal, layer_into, ngp_query_into, poison_, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
L, F = 16, 2
RES = O.hashgrid_resolutions(16, 16, 2048)
SCALE, OFFSET = 1.0 / (2.0 * 1.5), 0.5                       # HashNeRF(bound=1.5)
BIG = 8 * 256 * 3 + 5                                        # several tiles per wave
SHAPES = [(1, 1), (11, 3), (257, 1), (143, 43)]              # (B, n): M = 1, 33, 257, 8 * 256 * 3 + 5
GROUPS = [(0, 4), (4, 8), (8, 12), (12, 16), (0, 16)]
assert 143 * 43 == BIG and RES[4] <= 64 < RES[5]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _ires():
    return (C.c_int * L)(*[int(r) for r in RES])


def _cw(w):
    return (C.c_float * L)(*[float(v) for v in w])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _generic_w(seed):
    """random in (0, 1) with a few exact 0s and 1s, on both the LDS-combined and the hashed levels"""
    w = np.random.default_rng(seed).uniform(0.05, 0.95, L).astype(f32)
    w[[1, 6, 13]] = 0.0
    w[[0, 3, 9, 15]] = 1.0
    return w


def _pow2_w(seed, binary=False):
    rng = np.random.default_rng(seed)
    w = rng.choice([0.0, 1.0] if binary else [0.0, 0.25, 0.5, 1.0], L).astype(f32)
    w[[2, 11]] = 0.0
    w[[0, 14]] = 1.0
    if not binary:
        w[[4, 8]] = (0.25, 0.5)
    return w


def _rays(B, n, seed):
    """rays [B, 11] into the [-1.5, 1.5] box (a few origins beyond it), z [B, n] sorted depths"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.6, 1.6, (B, 3))
    d = rng.standard_normal((B, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((B, 1), 2.0), np.full((B, 1), 6.0), d], 1).astype(f32)
    z = np.sort(rng.uniform(0.0, 1.0, (B, n)), 1).astype(f32)
    return rays, z


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------------------------ 1. stand-alone encoders
@pytest.mark.parametrize("B,n", SHAPES)
def test_encoders_are_bit_exact(B, n):
    M = B * n
    rng = np.random.default_rng(M)
    w = _generic_w(M)
    T = 1 << 12
    tables = rng.standard_normal((L, T, F)).astype(f32)
    tables[w == 0] = np.nan                                  # never read
    rays, z = _rays(B, n, M)
    p = R.points(rays, z.reshape(-1), n, SCALE, OFFSET)
    want = LR.encode(p, tables, RES, w)
    td, pd, rd, zd = _dev(tables), _dev(p), _dev(rays), _dev(z)
    out = sentinel_(torch.empty(M, L * F, dtype=torch.float32, device=DEV))
    N.check(N.lib().nerf_hashgrid_forward_lw(N.ptr(pd), M, N.ptr(td), L, 12, F, _ires(), _cw(w), N.ptr(out), N.stream()))
    assert unwritten(out) == 0
    assert _eq_bits(_host(out), want)
    x = sentinel_(torch.empty(M, L * F + 16, dtype=torch.float32, device=DEV))
    pts = sentinel_(torch.empty(M, 3, dtype=torch.float32, device=DEV))
    N.check(N.lib().nerf_ngp_encode_lw(N.ptr(rd), N.ptr(zd), B, n, N.ptr(td), L, 12, F, _ires(), _cw(w), 3, SCALE, OFFSET,
                                       N.ptr(x), N.ptr(pts), N.stream()))
    assert unwritten(x) == 0 and unwritten(pts) == 0
    got = _host(x)
    assert _eq_bits(got[:, :L * F], want)
    assert _eq_bits(got[:, L * F:], R.sh(rays[np.arange(M) // n, 8:11], 3))
    assert _eq_bits(_host(pts), p)
    # NULL weights: the entry without the suffix
    clean = np.where(np.isnan(tables), f32(0.5), tables)
    cd = _dev(clean)
    a = sentinel_(torch.empty(M, L * F, dtype=torch.float32, device=DEV))
    N.check(N.lib().nerf_hashgrid_forward_lw(N.ptr(pd), M, N.ptr(cd), L, 12, F, _ires(), None, N.ptr(a), N.stream()))
    assert _eq_bits(_host(a), R.encode(p, clean, RES))


def test_entries_refuse_bad_weights():
    t = torch.zeros(L, 1 << 4, F, device=DEV)
    x = torch.zeros(4, 3, device=DEV)
    out = torch.zeros(4, L * F, device=DEV)
    for bad in (float("nan"), -0.5, 1.5, float("inf")):
        w = np.ones(L, f32)
        w[5] = bad
        with pytest.raises(ValueError, match="level weights"):
            N.check(N.lib().nerf_hashgrid_forward_lw(N.ptr(x), 4, N.ptr(t), L, 4, F, _ires(), _cw(w), N.ptr(out), N.stream()))


# ------------------------------------------------------------------------------------------------------------ 2. fused query
def _field(precision, half, seed=3, log2_t=12):
    from nerf_meets_mlx_amd.engine.ngp import HashNeRF
    f = HashNeRF(device=DEV, seed=seed, log2_hashmap_size=log2_t, precision=precision, half_tables=half)
    g = torch.Generator(device="cpu").manual_seed(seed)
    mag = torch.exp2(-8.0 * torch.rand(f.enc.tables.shape, generator=g))                  # [2^-8, 1]
    sign = torch.where(torch.rand(f.enc.tables.shape, generator=g) < 0.5, -1.0, 1.0)
    f.enc.tables.copy_((mag * sign).to(DEV))
    return f


def _scaled_tables(tables, w):
    """level l times w[l] (exact for powers of two); masked levels +0"""
    wt = torch.from_numpy(np.asarray(w, f32)).to(tables.device)
    out = tables * wt[:, None, None]
    out[wt == 0] = 0.0
    return out


MODES = [(22, False), (16, False), (16, True)]
QUERY_SHAPES = SHAPES + [(40, 3)]                            # ray-major inference tiling: B >= 32


@pytest.mark.parametrize("precision,half", MODES)
@pytest.mark.parametrize("train", [False, True])
def test_fused_query_equals_todays_kernels_on_scaled_tables(precision, half, train):
    f = _field(precision, half)
    w = _pow2_w(precision + half, binary=half)
    base = f.enc.tables.clone()
    scaled = _scaled_tables(base, w)
    shapes = QUERY_SHAPES + ([] if train else [(2048 * 256 + 300, 1)])     # inference: the grid-stride loop runs twice
    for B, n in shapes:
        rays, z = (_dev(a) for a in _rays(B, n, B * n))
        f.enc.tables.copy_(base)
        f.level_weights = w
        got = f.query(rays, z, train=train, fused=True).clone()
        f.enc.tables.copy_(scaled)
        f.level_weights = None
        want = f.query(rays, z, train=train, fused=True)
        assert not torch.isnan(got).any()
        assert bits_equal(got, want), (B, n)


@pytest.mark.parametrize("precision", [22, 16])
def test_fused_equals_unfused_with_weights(precision):
    f = _field(precision, False)
    f.level_weights = _generic_w(precision)
    for B, n in QUERY_SHAPES:
        rays, z = (_dev(a) for a in _rays(B, n, 7 * B + n))
        for train in (False, True):
            a = f.query(rays, z, train=train, fused=True).clone()
            b = f.query(rays, z, train=train, fused=False)
            assert torch.equal(a, b), (B, n, train)
    # the two row builders agree too, and follow the reference
    rays_h, z_h = _rays(11, 3, 5)
    rays, z = _dev(rays_h), _dev(z_h)
    _, x1 = f.features(rays, z)
    _, x2 = f.features_unfused(rays, z)
    assert bits_equal(x1, x2)
    p = R.points(rays_h, z_h.reshape(-1), 3, SCALE, OFFSET)
    assert _eq_bits(_host(x1)[:, :32], LR.encode(p, _host(f.enc.tables), RES, f.level_weights))


# ------------------------------------------------------------------------------------------------- 3. masked levels read nothing
@pytest.mark.parametrize("precision,half", MODES)
def test_masked_levels_are_not_read(precision, half):
    f = _field(precision, half)
    w = _pow2_w(17, binary=True) if half else _generic_w(17)
    f.level_weights = w
    base = f.enc.tables.clone()
    zeroed, poisoned = base.clone(), base.clone()
    zeroed[torch.from_numpy(w == 0)] = 0.0
    poisoned[torch.from_numpy(w == 0)] = float("nan")
    for B, n in QUERY_SHAPES:
        rays, z = (_dev(a) for a in _rays(B, n, 3 * B + n))
        outs = []
        for t in (zeroed, poisoned):
            f.enc.tables.copy_(t)
            o = [f.query(rays, z, fused=True).clone(), f.query(rays, z, train=True, fused=True).clone(),
                 f.features(rays, z)[1].clone()]
            if not half:
                o += [f.query(rays, z, fused=False).clone(), f.features_unfused(rays, z)[1].clone()]
            outs.append(o)
        for a, b in zip(*outs):
            assert not torch.isnan(b).any() and bits_equal(a, b), (B, n)


# ------------------------------------------------------------------------------------------------------------ 4. table gradient
SENT64 = 0x0123456789ABCDEF


def _scatter(rays, z, d_out, w, lo, hi, fixed, prefill, log2_t=12):
    acc = prefill.clone()
    B, n = z.shape
    if w is None:
        N.check(N.lib().nerf_hashgrid_backward_rays_ex(N.ptr(rays), N.ptr(z), B, n, N.ptr(d_out), L, log2_t, F, _ires(), SCALE,
                                                       OFFSET, lo, hi, int(fixed), N.ptr(acc), N.stream()))
    else:
        N.check(N.lib().nerf_hashgrid_backward_rays_ex_lw(N.ptr(rays), N.ptr(z), B, n, N.ptr(d_out), L, log2_t, F, _ires(), _cw(w),
                                                          SCALE, OFFSET, lo, hi, int(fixed), N.ptr(acc), N.stream()))
    torch.cuda.synchronize()
    return acc


@pytest.mark.parametrize("lo,hi", GROUPS)
@pytest.mark.parametrize("B,n", SHAPES)
def test_fixed_point_scatter_equals_premultiplied_gradient(B, n, lo, hi):
    M = B * n
    rng = np.random.default_rng(M + lo)
    w = _generic_w(M + lo)
    rays_h, z_h = _rays(B, n, M)
    d_h = rng.standard_normal((M, L * F)).astype(f32)
    rays, z, d_out, d_pre = _dev(rays_h), _dev(z_h), _dev(d_h), _dev(LR.premultiplied(d_h, w, L, F))
    T = 1 << 12
    prefill = torch.full((L, T, F), SENT64, dtype=torch.int64, device=DEV)
    got = _scatter(rays, z, d_out, w, lo, hi, True, prefill)
    want = _scatter(rays, z, d_pre, None, lo, hi, True, prefill)
    assert torch.equal(got, want)
    untouched = [l for l in range(L) if w[l] == 0 or not lo <= l < hi]
    assert (got[untouched] == SENT64).all()                  # masked levels (and the levels outside the range) keep the sentinel
    touched = [l for l in range(lo, hi) if w[l] != 0]
    assert all((got[l] != SENT64).any() for l in touched)
    if (B, n) == (11, 3):                                    # and against the host sum of the reference's addends
        p = R.points(rays_h, z_h.reshape(-1), n, SCALE, OFFSET)
        idx, val = LR.addends(p, d_h, RES, T, F, L, w, levels=range(lo, hi))
        ref = R.scatter_fixed(idx, R.to_fixed(val), L * T * F, prefill=np.full(L * T * F, SENT64, np.int64))
        assert np.array_equal(_host(got).reshape(-1), ref)
    # the point-list entry
    p_d = _dev(R.points(rays_h, z_h.reshape(-1), n, SCALE, OFFSET))
    acc = prefill.clone()
    N.check(N.lib().nerf_hashgrid_backward_ex_lw(N.ptr(p_d), M, N.ptr(d_out), L, 12, F, _ires(), _cw(w), lo, hi, 1, N.ptr(acc),
                                                 N.stream()))
    torch.cuda.synchronize()
    assert torch.equal(acc, got)


@pytest.mark.parametrize("lo,hi", GROUPS)
def test_float_scatter_of_one_sample(lo, hi):
    """One sample: no two addends of one instruction share an entry's word, so the float-atomic sums are exact too."""
    w = _pow2_w(lo, binary=True)
    rays_h, z_h = _rays(1, 1, 99)
    rays_h[0, 0:3] = (0.31, -0.47, 0.73)
    d_h = np.random.default_rng(lo).standard_normal((1, L * F)).astype(f32)
    rays, z, d_out, d_pre = _dev(rays_h), _dev(z_h), _dev(d_h), _dev(LR.premultiplied(d_h, w, L, F))
    prefill = torch.full((L, 1 << 12, F), 0.75, dtype=torch.float32, device=DEV)
    got = _scatter(rays, z, d_out, w, lo, hi, False, prefill)
    want = _scatter(rays, z, d_pre, None, lo, hi, False, prefill)
    assert bits_equal(got, want)
    untouched = [l for l in range(L) if w[l] == 0 or not lo <= l < hi]
    assert (got[untouched] == 0.75).all()


def _check_field_backward(f, w, d_raw_k):
    """After f.backward(): the table accumulators equal the existing entry fed the pre-multiplied d_x, group by group."""
    g_tab = f.enc.grad.clone()
    rays, z = f._rz
    _, d_x = f.mlp.backward(d_raw_k, need_input_grad=True)
    d_pre = _dev(LR.premultiplied(_host(d_x), w, L, F))
    want = torch.zeros_like(g_tab)
    for lo, hi in f.level_groups:
        want = _scatter(rays, z, d_pre, None, lo, hi, True, want)
    assert torch.equal(g_tab, want)
    assert (g_tab[torch.from_numpy(w == 0)] == 0).all() and (g_tab[torch.from_numpy(w != 0)] != 0).any()


@pytest.mark.parametrize("precision", [22, 16])
def test_field_backward_after_packed_and_culled_queries(precision):
    from nerf_meets_mlx_amd.engine.occupancy import OccupancyGrid, gather_rows
    f = _field(precision, False)
    w = _generic_w(precision)
    # packed: K rows, one depth each
    rays_h, z_h = _rays(300, 1, 21)
    rows, z = _dev(rays_h), _dev(z_h.reshape(-1))
    f.level_weights = w
    raw = f.query_packed(rows, z, train=True)
    f.level_weights = None                                   # backward() follows the weights of the query, not the property
    d_raw = _dev(np.random.default_rng(1).standard_normal((300, 1, 4)).astype(f32))
    f.backward(d_raw)
    _check_field_backward(f, w, d_raw)
    # culled: B x n samples, the kept ones only
    grid = OccupancyGrid(f, 2.0, 6.0, 8, seed=0, device=DEV)
    rays_h, z_h = _rays(40, 8, 22)
    rays, z = _dev(rays_h), _dev(z_h * 3.0)
    f.level_weights = w
    raw = f.query(rays, z, train=True, grid=grid)
    idx = f._sel[0].clone()
    assert 0 < idx.numel() < 40 * 8
    f.level_weights = None
    d_raw = _dev(np.random.default_rng(2).standard_normal((40, 8, 4)).astype(f32))
    f.backward(d_raw)
    _check_field_backward(f, w, gather_rows(d_raw.reshape(-1, 4), idx))
    # and with no weights at the query, none at the backward
    raw = f.query(rays, z, train=True, grid=grid)
    f.level_weights = w
    f.backward(d_raw)
    assert (f.enc.grad[1] != 0).any()                        # level 1 has w = 0 in `w`
    f.level_weights = None


# ---------------------------------------------------------------------------------------------------------------- 5 - 8. trainer
@pytest.fixture(scope="module")
def dataset():
    from nerf_meets_mlx_amd.dataset import synthetic
    imgs, poses, rposes, hwf, K = synthetic.make_dataset(16, 16, 5, seed=0, device=DEV)
    return imgs, poses, K


def _trainer(dataset, level_anneal, precision=22, **kw):
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    imgs, poses, K = dataset
    kw.setdefault("occupancy_grid", True)
    kw.setdefault("march_steps", 64)
    return NGPTrainer(imgs[:4], poses[:4], K, N_rand=64, n_depth_samples=64, seed=4, device=DEV, log2_hashmap_size=14,
                      precision=precision, level_anneal=level_anneal, **kw)


def _state(tr):
    f = tr.field
    return [f.mlp.params.clone(), f.enc.tables.clone()] + [t.clone() for k in ("mlp", "tables") for t in tr.opt.state[k]]


def _frame(tr, dataset):
    from nerf_meets_mlx_amd.rendering import ray
    _, poses, K = dataset
    rays = ray.gen_rays(16, 16, K, poses[4][:3, :4], 2.0, 6.0, torch.arange(256, device=DEV, dtype=torch.int64))
    return tr.render_rays(rays)


def test_all_ones_schedule_equals_no_schedule(dataset):
    a, b = _trainer(dataset, None), _trainer(dataset, (16, 10))
    for it in range(20):
        a.train_step()
        b.train_step()
        assert b.field.level_weights == ((1.0,) * 16 if it + 1 < 10 else None)
    for x, y in zip(_state(a), _state(b)):
        assert bits_equal(x, y)
    assert bits_equal(a.grid.density, b.grid.density)


@pytest.mark.parametrize("precision,kw", [(22, {}), (16, {}), (22, dict(march_steps=None)),
                                          (22, dict(march_steps=None, occupancy_grid=False)),
                                          (22, dict(march_steps=None, occupancy_grid=False, bound=None))])
def test_masked_tables_do_not_move(dataset, precision, kw):
    tr = _trainer(dataset, (4, 40), precision=precision, **kw)
    assert tr.field.level_weights == (1.0,) * 4 + (0.0,) * 12
    t0 = tr.field.enc.tables.clone()
    for _ in range(10):
        tr.train_step()
    first_masked = int(np.ceil(4 + 12 * 9 / 40))             # alpha(9) = 6.7: levels 7 ... 15 were never active
    assert first_masked == 7
    t1 = tr.field.enc.tables
    assert bits_equal(t1[first_masked:], t0[first_masked:])
    assert all(not bits_equal(t1[l], t0[l]) for l in range(4))
    n = t0.numel()
    moments = [t for t in tr.opt.state["tables"] if torch.is_tensor(t) and t.numel() == n]
    assert len(moments) == 2
    for m in moments:
        assert (m.view(L, -1)[first_masked:] == 0).all() and (m.view(L, -1)[:4] != 0).any()
    assert tr.field.level_weights == tr.level_weights_at(10) == (1.0,) * 7 + (0.0,) * 9      # alpha(10) = 7: the current `it`
    for _ in range(30):
        tr.train_step()
    assert tr.it == 40 and tr.field.level_weights is None and tr.level_weights_at(40) is None
    assert not bits_equal(tr.field.enc.tables[15], t0[15])   # every level trains in the end


def test_resume_follows_the_restored_iteration(dataset, tmp_path):
    a = _trainer(dataset, (4, 40))
    for _ in range(15):
        a.train_step()
    path = a.save(str(tmp_path / "ckpt"))
    b = _trainer(dataset, (4, 40))
    assert b.load(path) == 15
    assert b.field.level_weights == a.field.level_weights == a.level_weights_at(15)
    for _ in range(10):
        a.train_step()
        b.train_step()
    for x, y in zip(_state(a), _state(b)):
        assert bits_equal(x, y)
    assert bits_equal(_frame(a, dataset), _frame(b, dataset))


def test_rendering_and_density_volume_see_the_weights(dataset):
    a, b = _trainer(dataset, (4, 40)), _trainer(dataset, None)
    with torch.no_grad():                                    # tables large enough for a frame that is not the background
        big = _field(22, False, seed=4, log2_t=14).enc.tables
        a.field.enc.tables.copy_(big)
        b.field.enc.tables.copy_(big)
        b.field.enc.tables[4:] = 0.0
    assert a.field.level_weights == (1.0,) * 4 + (0.0,) * 12 and b.field.level_weights is None
    fa, fb = _frame(a, dataset), _frame(b, dataset)
    assert bits_equal(fa, fb)
    va, vb = a.density_volume(16), b.density_volume(16)
    assert bits_equal(va, vb) and float(va.std()) > 0
    c = _trainer(dataset, None)                              # and the weights matter: all 16 levels give another volume
    c.field.enc.tables.copy_(big)
    assert not bits_equal(c.density_volume(16), va)


# ----------------------------------------------------------------------- 9. a plain entry is its `_lw` entry with NULL weights
# M = 300: one full 256-thread block plus a tail; for the write-combining kernel four full 64-sample chunks plus a tail.  With
# hash_combine_max_res = 64 three levels go through LDS and three direct, and a group of 4 levels per thread straddles that line.
PAIR_RES = [16, 30, 64, 65, 181, 2048]
PAIR_L, PAIR_B, PAIR_N, PAIR_LOG2_T = 6, 100, 3, 12
PAIR_M = PAIR_B * PAIR_N
PAIR_PATHS = [(1, 0), (2, 0), (4, 0), (8, 0), (2, 64), (4, 64)]          # (F, hash_combine_max_res): 0 = every level direct


@contextlib.contextmanager
def _combine(max_res):
    lib = N.lib()
    old = lib.nerf_get_option(b"hash_combine_max_res")
    N.check(lib.nerf_set_option(b"hash_combine_max_res", int(max_res)))
    try:
        yield
    finally:
        N.check(lib.nerf_set_option(b"hash_combine_max_res", old))


@pytest.fixture(scope="module")
def pair_points():
    """(rays [B, 11], z [B, n], the same M = B n points as a list [M, 3]) on the device"""
    rays, z = _rays(PAIR_B, PAIR_N, 77)
    return _dev(rays), _dev(z), _dev(R.points(rays, z.reshape(-1), PAIR_N, SCALE, OFFSET))


@pytest.mark.parametrize("Fp", [1, 2, 4, 8])
def test_plain_encoders_equal_the_lw_entries_with_null(Fp, pair_points):
    rays, z, p = pair_points
    lib, s, res = N.lib(), N.stream(), (C.c_int * PAIR_L)(*PAIR_RES)
    M, L, lt = PAIR_M, PAIR_L, PAIR_LOG2_T
    tables = _dev(np.random.default_rng(Fp).standard_normal((L, 1 << lt, Fp)).astype(f32))
    outs = []
    for lw in (False, True):
        out = sentinel_(torch.empty(M, L * Fp, dtype=torch.float32, device=DEV))
        x = sentinel_(torch.empty(M, L * Fp + 16, dtype=torch.float32, device=DEV))
        pts = sentinel_(torch.empty(M, 3, dtype=torch.float32, device=DEV))
        if lw:
            N.check(lib.nerf_hashgrid_forward_lw(N.ptr(p), M, N.ptr(tables), L, lt, Fp, res, None, N.ptr(out), s))
            N.check(lib.nerf_ngp_encode_lw(N.ptr(rays), N.ptr(z), PAIR_B, PAIR_N, N.ptr(tables), L, lt, Fp, res, None, 3, SCALE,
                                           OFFSET, N.ptr(x), N.ptr(pts), s))
        else:
            N.check(lib.nerf_hashgrid_forward(N.ptr(p), M, N.ptr(tables), L, lt, Fp, res, N.ptr(out), s))
            N.check(lib.nerf_ngp_encode(N.ptr(rays), N.ptr(z), PAIR_B, PAIR_N, N.ptr(tables), L, lt, Fp, res, 3, SCALE, OFFSET,
                                        N.ptr(x), N.ptr(pts), s))
        outs.append((out, x, pts))
    for a, b in zip(*outs):
        assert unwritten(a) == 0 and unwritten(b) == 0 and bits_equal(a, b)
    assert bits_equal(outs[0][0], outs[0][1][:, :L * Fp])


@pytest.mark.parametrize("Fp,combine", PAIR_PATHS)
def test_plain_scatters_equal_the_lw_entries_with_null(Fp, combine, pair_points):
    """Fixed-point mode only: float atomics are not order-independent.  Random int64 in every accumulator; all bytes compared."""
    rays, z, p = pair_points
    lib, s, res = N.lib(), N.stream(), (C.c_int * PAIR_L)(*PAIR_RES)
    M, L, lt = PAIR_M, PAIR_L, PAIR_LOG2_T
    rng = np.random.default_rng(10 * Fp + combine)
    d_out = _dev(rng.standard_normal((M, L * Fp)).astype(f32))
    prefill = _dev(rng.integers(-(1 << 62), 1 << 62, (L, 1 << lt, Fp), dtype=np.int64))
    pts, pts_lw, ray, ray_lw = (prefill.clone() for _ in range(4))
    with _combine(combine):
        N.check(lib.nerf_hashgrid_backward_ex(N.ptr(p), M, N.ptr(d_out), L, lt, Fp, res, 0, L, 1, N.ptr(pts), s))
        N.check(lib.nerf_hashgrid_backward_ex_lw(N.ptr(p), M, N.ptr(d_out), L, lt, Fp, res, None, 0, L, 1, N.ptr(pts_lw), s))
        N.check(lib.nerf_hashgrid_backward_rays_ex(N.ptr(rays), N.ptr(z), PAIR_B, PAIR_N, N.ptr(d_out), L, lt, Fp, res, SCALE,
                                                   OFFSET, 0, L, 1, N.ptr(ray), s))
        N.check(lib.nerf_hashgrid_backward_rays_ex_lw(N.ptr(rays), N.ptr(z), PAIR_B, PAIR_N, N.ptr(d_out), L, lt, Fp, res, None,
                                                      SCALE, OFFSET, 0, L, 1, N.ptr(ray_lw), s))
        torch.cuda.synchronize()
    assert torch.equal(pts, pts_lw) and torch.equal(ray, ray_lw) and torch.equal(pts, ray)
    assert all((pts[l] != prefill[l]).any() for l in range(L))           # every level was scattered into


def _query_lw_null(f, rays, z, train):
    """tests/_poison.py:ngp_query_into through `nerf_ngp_query_fused_lw` with NULL weights"""
    B, n = z.shape
    e, m = f.enc, f.mlp
    raw = sentinel_(torch.empty(B, n, 4, dtype=torch.float32, device=z.device))
    acts = poison_(m._begin_train_pass(B * n), NAN_BYTES) if train else None
    N.check(N.lib().nerf_ngp_query_fused_lw(C.byref(m.arch), N.ptr(m.packed()), N.ptr(rays), N.ptr(z), B, n, N.ptr(e.tables),
                                            N.ptr(f.table.shadow()), e.n_levels, e.log2_hashmap_size, e.n_features_per_level,
                                            e._res_c, None, 3, f.pos_scale, f.pos_offset, N.ptr(raw), N.ptr(acts), N.stream()))
    return raw


@pytest.mark.parametrize("precision,half", MODES)
@pytest.mark.parametrize("train", [False, True])
def test_plain_fused_query_equals_the_lw_entry_with_null(precision, half, train):
    f = _field(precision, half)
    rays, z = (_dev(a) for a in _rays(40, 3, 120))
    layers = (0, 1, 9) if train else ()                                  # the stored activations of the 2 x 64 model
    want = ngp_query_into(f, rays, z, NAN_BYTES, train=train)            # nerf_ngp_query_fused_h
    want_acts = [layer_into(f.mlp, "acts", l) for l in layers]
    got = _query_lw_null(f, rays, z, train)
    got_acts = [layer_into(f.mlp, "acts", l) for l in layers]
    assert unwritten(want) == 0 and unwritten(got) == 0 and bits_equal(got, want)
    for a, b in zip(got_acts, want_acts):
        assert unwritten(a) == 0 and bits_equal(a, b)
    assert bits_equal(f.query(rays, z, train=train, fused=True), want)   # HashNeRF.query with level_weights None: the same call


def test_error_texts_name_the_entry_that_was_called():
    """Codes and texts as the entries gave them before they shared their bodies."""
    lib, s = N.lib(), N.stream()
    res = (C.c_int * 4)(16, 16, 16, 16)
    x = torch.zeros(8, 3, device=DEV)
    t = torch.zeros(4, 16, 8, device=DEV)
    out = torch.zeros(8, 64, device=DEV)
    acc = torch.zeros(4, 16, 8, dtype=torch.int64, device=DEV)
    rays, z = torch.zeros(2, 11, device=DEV), torch.zeros(2, 4, device=DEV)
    X, T, O_, A, G, Rp, Z = (N.ptr(a) for a in (x, t, out, acc, out, rays, z))
    E_UNSUP = -3
    cases = [
        (lambda: lib.nerf_hashgrid_forward(X, 8, T, 4, 4, 3, res, O_, s), b"nerf_hashgrid_forward: F must be 1, 2, 4 or 8"),
        (lambda: lib.nerf_hashgrid_forward_lw(X, 8, T, 4, 4, 3, res, None, O_, s),
         b"nerf_hashgrid_forward_lw: F must be 1, 2, 4 or 8"),
        (lambda: lib.nerf_ngp_encode(Rp, Z, 2, 4, T, 4, 4, 3, res, 2, 1.0, 0.0, O_, None, s),
         b"nerf_ngp_encode: F must be 1, 2, 4 or 8"),
        (lambda: lib.nerf_ngp_encode_lw(Rp, Z, 2, 4, T, 4, 4, 3, res, None, 2, 1.0, 0.0, O_, None, s),
         b"nerf_ngp_encode_lw: F must be 1, 2, 4 or 8"),
        (lambda: lib.nerf_hashgrid_backward_ex(X, 8, G, 4, 4, 2, res, 0, 4, 2, A, s),
         b"nerf_hashgrid_backward_ex: fixed_point must be 0 or 1"),
        (lambda: lib.nerf_hashgrid_backward_ex_lw(X, 8, G, 4, 4, 2, res, None, 0, 4, 2, A, s),
         b"nerf_hashgrid_backward_ex_lw: fixed_point must be 0 or 1"),
        (lambda: lib.nerf_hashgrid_backward_rays_ex(Rp, Z, 2, 4, G, 4, 4, 2, res, 1.0, 0.0, 0, 4, 2, A, s),
         b"nerf_hashgrid_backward_rays_ex: fixed_point must be 0 or 1"),
        (lambda: lib.nerf_hashgrid_backward_rays_ex_lw(Rp, Z, 2, 4, G, 4, 4, 2, res, None, 1.0, 0.0, 0, 4, 2, A, s),
         b"nerf_hashgrid_backward_rays_ex_lw: fixed_point must be 0 or 1"),
    ]
    for call, text in cases:
        assert call() == E_UNSUP
        assert lib.nerf_last_error() == text
