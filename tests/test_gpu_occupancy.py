"""Occupancy-grid empty-space skipping for the hash-grid model (engine/occupancy.py, csrc/occupancy.hip) on the GPU.

Against the torch reference of tests/_occupancy_ref.py: the update (points, merge, threshold, pack), the cull / compaction; then
the culled query and backward against the full query, the trainer (warm-up bit-identity, kept fraction, PSNR), the checkpoint."""
import numpy as np
import pytest
import torch

from tests import _occupancy_ref as R
from tests._poison import PATTERNS, bits_equal, ngp_query_into, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _field(precision=22, seed=3):
    from nerf_meets_mlx_amd.engine.ngp import HashNeRF
    f = HashNeRF(device=DEV, seed=seed, log2_hashmap_size=14, precision=precision)
    f.enc.tables.normal_(0.0, 0.3, generator=torch.Generator(device=DEV).manual_seed(seed))
    if f.table.half is not None:
        f.table.mark_updated()
    return f


def _grid(f, seed=0):
    from nerf_meets_mlx_amd.engine.occupancy import OccupancyGrid
    return OccupancyGrid(f, 2.0, 6.0, 64, seed=seed)


def _set_bits(grid, occ):
    grid.bits.copy_(R.pack(occ.to(DEV)))


def _rays(B, seed, spread=2.0, inside=False):
    """rays [B, 11], z [B, n = 64]; inside=True keeps every sample strictly inside the [-1.5, 1.5]^3 box."""
    g = torch.Generator().manual_seed(seed)
    if inside:
        o = torch.rand(B, 3, generator=g) - 0.5
        zmax = 0.9
    else:
        o = (torch.rand(B, 3, generator=g) * 2 - 1) * spread
        zmax = 4.0
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1)
    rays = torch.cat([o, d, torch.zeros(B, 2), d], 1).float().contiguous()
    z = torch.sort(torch.rand(B, 64, generator=g) * zmax, dim=1).values.contiguous()
    return rays.to(DEV), z.to(DEV)


# ------------------------------------------------------------------------------------------------ 1: points, merge, finalize
def test_points_lie_in_their_cells_and_are_reproducible():
    from nerf_meets_mlx_amd.engine.occupancy import LOG2_RES, RES
    f = _field()
    g = _grid(f, seed=11)
    rays, z = g.points(5)
    assert rays.shape == (RES ** 3, 11) and z.shape == (RES ** 3, 1)
    assert torch.equal(rays[:, 3:], torch.zeros_like(rays[:, 3:])) and torch.equal(z, torch.zeros_like(z))
    cells = R.cell_index(R.unit_coords(rays, z, g.pos_scale, g.pos_offset)[:, 0], LOG2_RES)
    assert torch.equal(cells, torch.arange(RES ** 3, device=DEV))
    again, _ = g.points(5)
    assert bits_equal(rays, again)
    part, _ = g.points(5, cell0=12345, count=1000)
    assert bits_equal(part, rays[12345:13345])
    other, _ = g.points(6)
    g2 = _grid(f, seed=12)
    other_seed, _ = g2.points(5)
    # jittered: far from the cell centres, and a different stream per update and per seed
    assert float((other[:, :3] != rays[:, :3]).float().mean()) > 0.99
    assert float((other_seed[:, :3] != rays[:, :3]).float().mean()) > 0.99


def test_merge_and_finalize_match_the_reference():
    from nerf_meets_mlx_amd.engine.occupancy import RES
    f = _field()
    g = _grid(f)
    gen = torch.Generator(device=DEV).manual_seed(1)
    n = RES ** 3
    density = torch.rand(n, device=DEV, generator=gen) * 0.3
    g.density.copy_(density)
    want = density.clone()
    for step in range(3):
        raw = torch.randn(n, 4, device=DEV, generator=gen) * 0.2
        raw[::9973, 3] = float("nan")
        raw[::10007, 3] = float("-inf")
        g.merge(raw)
        want = R.merge(want, raw[:, 3])
        assert bits_equal(g.density, want), step
    g._finalize()
    thr = R.threshold(want, g.thr_cap)
    assert abs(float(g.thr) - float(thr)) <= float(torch.finfo(torch.float32).eps) * float(thr)
    got = R.unpack(g.bits)
    ref = R.occupancy(want, thr)
    near = (want - thr).abs() <= torch.finfo(torch.float32).eps * thr
    assert int(near.sum()) < 100
    assert torch.equal(got[~near], ref[~near])
    # the cap: a grid of large densities is thresholded at 0.01 / delta, delta = 4 / 64
    g.density.fill_(10.0)
    g.density[: n // 2] = 0.1
    g._finalize()
    assert float(g.thr) == np.float32(0.01 / (4.0 / 64))
    assert abs(g.occupied_fraction() - 0.5) < 1e-9


def test_update_uses_the_fields_density_at_the_points():
    """update() = points -> fused query (n = 1) -> merge -> finalize; sigma taken from the same rows by the plain query."""
    from nerf_meets_mlx_amd.engine.occupancy import RES
    f = _field()
    g = _grid(f, seed=2)
    assert g.occupied_fraction() == 1.0                      # starts all occupied
    g.update(f, 16 * 7)
    rays, z = g.points(7)
    sigma = torch.cat([f.query(rays[s:s + (1 << 19)], z[s:s + (1 << 19)])[:, 0, 3] for s in range(0, RES ** 3, 1 << 19)])
    want = R.merge(torch.zeros(RES ** 3, device=DEV), sigma)
    assert bits_equal(g.density, want)
    frac = g.occupied_fraction()
    assert 0.0 < frac < 1.0 and g.updates == 1


def test_grid_needs_a_scene_box():
    from nerf_meets_mlx_amd.engine.ngp import HashNeRF
    f = HashNeRF(device=DEV, seed=0, log2_hashmap_size=14, bound=None)
    with pytest.raises(ValueError):
        _grid(f)


# ------------------------------------------------------------------------------------------------ 2: cull
@pytest.mark.parametrize("case", ["random", "empty", "full", "odd", "large"])
def test_cull_matches_nonzero(case):
    from nerf_meets_mlx_amd.engine.occupancy import LOG2_RES, RES
    f = _field()
    g = _grid(f)
    B, n = {"odd": (37, 29), "large": (17000, 64)}.get(case, (500, 64))
    rays, z = _rays(B, 7)
    z = z[:, :n].contiguous()
    occ = {"empty": torch.zeros(RES ** 3, dtype=torch.bool), "full": torch.ones(RES ** 3, dtype=torch.bool)}.get(
        case, torch.rand(RES ** 3, generator=torch.Generator().manual_seed(3)) < 0.3)
    _set_bits(g, occ)
    mask = R.keep_mask(rays, z, occ.to(DEV), LOG2_RES, g.pos_scale, g.pos_offset)
    assert B * n > 2 ** 20 if case == "large" else True
    assert bool((~mask).any())                               # samples outside the box are culled even by a full grid
    raw = sentinel_(torch.empty(B, n, 4, device=DEV))
    idx, rk, zk, raw, K = g.cull(rays, z, raw=raw)
    want = torch.nonzero(mask.reshape(-1)).reshape(-1)
    assert K == want.numel() and torch.equal(idx, want)
    if case == "empty":
        assert K == 0
    assert bits_equal(rk, rays[want // n]) and bits_equal(zk.reshape(-1), z.reshape(-1)[want])
    flat = raw.reshape(-1, 4)
    culled = torch.ones(B * n, dtype=torch.bool, device=DEV)
    culled[want] = False
    assert torch.equal(flat[culled], torch.zeros_like(flat[culled]))
    assert unwritten(flat[~culled]) == 4 * K                  # the kept rows are left for the scatter


# ------------------------------------------------------------------------------------------------ 3: query
@pytest.mark.parametrize("precision", [22, 16])
def test_culled_query_matches_the_full_query(precision):
    from nerf_meets_mlx_amd.engine.occupancy import LOG2_RES, RES, scatter_rows
    f = _field(precision)
    g = _grid(f)
    occ = torch.rand(RES ** 3, generator=torch.Generator().manual_seed(5)) < 0.5
    _set_bits(g, occ)
    rays, z = _rays(700, 9, spread=1.2)
    mask = R.keep_mask(rays, z, occ.to(DEV), LOG2_RES, g.pos_scale, g.pos_offset)
    assert 0 < int(mask.sum()) < mask.numel()
    for train in (False, True):
        full = f.query(rays, z, train=train).clone()
        got = f.query(rays, z, train=train, grid=g)
        assert bits_equal(got[mask], full[mask]), (precision, train)
        assert torch.equal(got[~mask], torch.zeros_like(got[~mask]))
        # the same composition on poisoned buffers: every element of raw is written, by the fill or by the scatter
        for pat in PATTERNS:
            idx, rk, zk, raw, K = g.cull(rays, z, raw=sentinel_(torch.empty(700, 64, 4, device=DEV)))
            raw_k = ngp_query_into(f, rk, zk, pat, train=train)
            assert unwritten(raw_k) == 0
            scatter_rows(raw_k, idx, raw)
            assert unwritten(raw) == 0 and bits_equal(raw, got), (precision, train, pat)
    # all-occupied grid, every sample inside the box: the whole tensor is the full query's
    _set_bits(g, torch.ones(RES ** 3, dtype=torch.bool))
    rays, z = _rays(300, 10, inside=True)
    assert bool(R.keep_mask(rays, z, torch.ones(RES ** 3, dtype=torch.bool, device=DEV), LOG2_RES, g.pos_scale, g.pos_offset).all())
    for train in (False, True):
        assert bits_equal(f.query(rays, z, train=train, grid=g), f.query(rays, z, train=train))


# ------------------------------------------------------------------------------------------------ 4: backward
def _grads(f, rays, z, d_raw, grid=None):
    f.query(rays, z, train=True, grid=grid)
    g_mlp, g_tab = f.backward(d_raw)
    return g_mlp.clone(), g_tab.clone()


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_culled_backward_matches_the_full_backward():
    from nerf_meets_mlx_amd.engine.occupancy import LOG2_RES, RES
    f = _field()
    assert f.deterministic
    g = _grid(f)
    occ = torch.rand(RES ** 3, generator=torch.Generator().manual_seed(6)) < 0.5
    _set_bits(g, occ)
    rays, z = _rays(1000, 12, spread=1.2)
    mask = R.keep_mask(rays, z, occ.to(DEV), LOG2_RES, g.pos_scale, g.pos_offset)
    d_raw = torch.randn(1000, 64, 4, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) * 1e-3
    d_masked = d_raw * mask[..., None]
    m_full, t_full = _grads(f, rays, z, d_masked)
    m_cull, t_cull = _grads(f, rays, z, d_raw, grid=g)
    assert t_cull.dtype == torch.int64 and torch.equal(t_cull, t_full)
    assert bool(t_full.ne(0).any())
    assert _rel_l2(m_cull, m_full) < 2e-6


def test_all_occupied_grid_gives_a_bit_identical_step():
    from nerf_meets_mlx_amd.engine.occupancy import RES
    f = _field()
    g = _grid(f)
    _set_bits(g, torch.ones(RES ** 3, dtype=torch.bool))
    rays, z = _rays(512, 13, inside=True)
    d_raw = torch.randn(512, 64, 4, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)) * 1e-3
    m_full, t_full = _grads(f, rays, z, d_raw)
    m_cull, t_cull = _grads(f, rays, z, d_raw, grid=g)
    assert bits_equal(m_cull, m_full) and torch.equal(t_cull, t_full)


def test_no_kept_sample_gives_zero_gradients():
    f = _field()
    g = _grid(f)
    g.bits.zero_()
    rays, z = _rays(256, 14)
    d_raw = torch.randn(256, 64, 4, device=DEV)
    _grads(f, rays, z, d_raw)                                # leaves nonzero gradients behind
    raw = f.query(rays, z, train=True, grid=g)
    assert torch.equal(raw, torch.zeros_like(raw))
    g_mlp, g_tab = f.backward(d_raw)
    assert not bool(g_mlp.ne(0).any()) and not bool(g_tab.ne(0).any())


# ------------------------------------------------------------------------------------------------ 5: trainer
def _trainers(hw, views, log2_t, seed, n_rand=1024, **kw):
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    imgs, poses, rposes, hwf, K = synthetic.make_dataset(hw, hw, views + 1, seed=0, device=DEV)
    mk = lambda grid: NGPTrainer(imgs[:-1], poses[:-1], K, N_rand=n_rand, n_depth_samples=64, seed=seed, device=DEV,
                                 log2_hashmap_size=log2_t, occupancy_grid=grid, **kw)
    return mk(False), mk(True), imgs[-1], poses[-1]


def _state(tr):
    f = tr.field
    return [f.mlp.params.clone(), f.enc.tables.clone()] + [t.clone() for k in ("mlp", "tables") for t in tr.opt.state[k]]


def test_trainer_warmup_is_bit_identical_then_culls_and_keeps_psnr():
    """hw 48, 2^14-entry tables, seed 4, 256 rays per step: the first 256 steps with the grid are the grid-free steps bit for bit
    (parameters, tables, Adam moments; the loss scalar is a float-atomic sum, equal to rounding); after them the grid culls a third
    of the training samples or more, the loss stays finite, and after 600 iterations the held-out PSNR is within 0.5 dB of the
    grid-free run.  (Measured at this size: kept 0.60-0.70 of the samples, PSNR +0.38 dB with the grid.)"""
    from nerf_meets_mlx_amd.engine.occupancy import WARMUP
    off, on, gt, pose = _trainers(48, 8, 14, 4, n_rand=256)
    for it in range(WARMUP):
        l_off, l_on = off.train_step()["loss_coarse"], on.train_step()["loss_coarse"]
    assert torch.allclose(l_on, l_off, rtol=1e-5, atol=0)
    for a, b in zip(_state(on), _state(off)):
        assert bits_equal(a, b)
    assert on.grid.updates == WARMUP // 16
    kept = []
    for it in range(WARMUP, 600):
        off.train_step()
        out = on.train_step()
        kept.append(on._field._sel[0].numel() / (256 * 64))
    assert np.isfinite(float(out["loss_coarse"]))
    assert max(kept[-100:]) < 0.75, (min(kept), max(kept))
    p_off, p_on = off.psnr(pose[:3, :4].numpy(), gt), on.psnr(pose[:3, :4].numpy(), gt)
    assert abs(p_on - p_off) < 0.5, (p_on, p_off)


# ------------------------------------------------------------------------------------------------ 6: checkpoint
def test_checkpoint_resume_is_bit_identical(tmp_path):
    from nerf_meets_mlx_amd.engine.occupancy import WARMUP
    _, a, _, _ = _trainers(32, 4, 14, 4)
    N = 2 * WARMUP + 68                                      # the save (N / 2 = 290) lies after the warm-up, between two updates
    for _ in range(N // 2):
        a.train_step()
    path = a.save(str(tmp_path / "ckpt"))
    bits_at_save = a.grid.bits.clone()
    assert "extra/occupancy/density" in np.load(path).files
    for _ in range(N - N // 2):
        a.train_step()
    _, b, _, _ = _trainers(32, 4, 14, 9)                     # another seed: load() must bring everything back
    assert b.load(path) == N // 2
    assert bits_equal(b.grid.bits, bits_at_save)                # the bitfield rebuilt from the saved density
    for _ in range(N - N // 2):
        b.train_step()
    for x, y in zip(_state(b), _state(a)):
        assert bits_equal(x, y)
    assert bits_equal(b.grid.density, a.grid.density) and bits_equal(b.grid.bits, a.grid.bits)


def test_checkpoint_without_grid_is_unchanged(tmp_path):
    off, _, _, _ = _trainers(32, 4, 14, 4)
    off.train_step()
    z = np.load(off.save(str(tmp_path / "off")))
    assert z.files and not [k for k in z.files if k.startswith("extra/")]
