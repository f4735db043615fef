"""Occupancy-guided ray march (engine/occupancy.py OccupancyGrid.march, csrc/occupancy.hip) and packed compositing
(csrc/composite_packed.hip) on the GPU, against the torch reference of tests/_march_ref.py: the march bit for bit, the packed
forward and MSE backward against float64, the exp merge; then the trainer in march mode (reproducibility, fewer samples after the
warm-up, a frame that is not white), checkpoint resume, and two ranks with different sample counts."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import _march_ref as M
from tests import _occupancy_ref as O
from tests._poison import bits_equal, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT64 = 0x7FE5A5A5A5A5A5A5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _field(seed=3):
    from nerf_meets_mlx_amd.engine.ngp import HashNeRF
    f = HashNeRF(device=DEV, seed=seed, log2_hashmap_size=14)
    f.enc.tables.normal_(0.0, 0.3, generator=torch.Generator(device=DEV).manual_seed(seed))
    return f


def _grid(f, steps):
    from nerf_meets_mlx_amd.engine.occupancy import OccupancyGrid
    return OccupancyGrid(f, 2.0, 6.0, 64, march_steps=steps)


def _rays(B, seed):
    """A mix: rays from outside through the box, rays starting inside, grazing rays along a face, axis-parallel rays, NaN rays."""
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(B, 3, generator=g) * 2 - 1) * 4.0
    tgt = (torch.rand(B, 3, generator=g) * 2 - 1) * 1.2
    d = torch.nn.functional.normalize(tgt - o, dim=-1)
    nf = torch.tensor([[2.0, 6.0]]).expand(B, 2).clone()
    q = B // 8
    o[:q] = (torch.rand(q, 3, generator=g) - 0.5) * 2.0          # inside the box, near = 0
    nf[:q, 0] = 0.0
    o[q:2 * q, 1] = 1.5                                          # grazing: on the y = +bound face, moving in x / z only ...
    d[q:2 * q, 1] = 1e-7                                         # ... with a tiny y component
    d[2 * q:2 * q + 4, 2] = 0.0                                  # axis-parallel
    o[2 * q + 4:2 * q + 6, 0] = float("nan")                     # NaN rays
    d[2 * q + 6, 1] = float("nan")
    d = d.clone()
    rays = torch.cat([o, d, nf, d], 1).float().contiguous()
    return rays.to(DEV)


def _march_poisoned(g, rays, jitter, use_bits):
    """OccupancyGrid.march with every output buffer filled with sentinels first (the capacity buffers are grown to the right size
    by a first call, then poisoned and the march repeated)."""
    g.march(rays, jitter, use_bits=use_bits)
    for k in ("march_offsets", "march_rows", "march_z"):
        t = g._cull[k]
        if t.dtype == torch.int64:
            t.fill_(SENT64)
        else:
            sentinel_(t)
    offs, rows, z, K = g.march(rays, jitter, use_bits=use_bits)
    return offs.clone(), rows.clone(), z.clone(), K


# ------------------------------------------------------------------------------------------------ 1: march
@pytest.mark.parametrize("steps", [1, 64, 1024])
@pytest.mark.parametrize("occ_case", ["empty", "full", "random", "one", "warmup"])
def test_march_matches_the_reference_bit_for_bit(steps, occ_case):
    from nerf_meets_mlx_amd.engine.occupancy import LOG2_RES, RES
    f = _field()
    g = _grid(f, steps)
    rays = _rays(512, 5)
    gen = torch.Generator().manual_seed(11)
    occ = {"empty": torch.zeros(RES ** 3, dtype=torch.bool), "full": torch.ones(RES ** 3, dtype=torch.bool),
           "random": torch.rand(RES ** 3, generator=gen) < 0.3, "warmup": torch.zeros(RES ** 3, dtype=torch.bool)}.get(occ_case)
    if occ_case == "one":
        occ = torch.zeros(RES ** 3, dtype=torch.bool)
        occ[64 + RES * (64 + RES * 64)] = True
    g.bits.copy_(O.pack(occ.to(DEV)))
    use_bits = occ_case != "warmup"
    jit_rays = torch.rand(512, generator=gen).float()
    for jitter in (0.0, 0.5, 1.0 - 2.0 ** -24, jit_rays):
        jd = jitter.to(DEV) if torch.is_tensor(jitter) else jitter
        offs, rows, z, K = _march_poisoned(g, rays, jd, use_bits)
        # the reference on the CPU: IEEE division and square root, one rounding per op
        w_offs, w_rows, w_z, w_K = M.march(rays.cpu(), jitter, occ if use_bits else None, LOG2_RES, g.pos_scale, g.pos_offset,
                                           g.step_world, steps)
        assert K == w_K and torch.equal(offs.cpu(), w_offs), (steps, occ_case, jitter if not torch.is_tensor(jitter) else "rays")
        assert bits_equal(z.cpu(), w_z) and bits_equal(rows.cpu(), w_rows)
        assert unwritten(z) == 0 and unwritten(rows) == 0 and not bool((offs == SENT64).any())
        if occ_case == "empty":
            assert K == 0
        if occ_case in ("full", "warmup") and (steps > 1 or (not torch.is_tensor(jitter) and jitter == 0.0)):  # one step of sqrt(3) 2 bound overshoots most chords
            assert K > 0
        # degenerate rays: axis-parallel and NaN rays get no sample
        cnt = offs[1:] - offs[:-1]
        assert int(cnt[128:135].sum()) == 0
        again = g.march(rays, jd, use_bits=use_bits)
        assert torch.equal(again[0], offs) and bits_equal(again[2], z) and bits_equal(again[1], rows)


def test_march_of_no_rays_and_of_rays_that_miss():
    f = _field()
    g = _grid(f, 64)
    offs, rows, z, K = g.march(torch.empty(0, 11, device=DEV), 0.5)
    assert K == 0 and offs.tolist() == [0]
    rays = _rays(64, 6)
    rays[:, 0:3] = 10.0                                          # outside, moving away from the box
    rays[:, 3:6] = 1.0
    offs, rows, z, K = g.march(rays, 0.5)
    assert K == 0 and offs.tolist() == [0] * 65


# ------------------------------------------------------------------------------------------------ 2, 3: packed compositing
def _packed(lengths, seed, sigmas=(-100.0, 0.0, 20.0, 100.0, 1e30)):
    g = torch.Generator().manual_seed(seed)
    offs = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    offs[1:] = torch.cumsum(torch.tensor(lengths), 0)
    K = int(offs[-1])
    raw = torch.rand(K, 4, generator=g)
    raw[:, 3] = torch.randn(K, generator=g) * 3.0
    z = torch.sort(torch.rand(K, generator=g) * 4 + 2).values
    # the special densities, each at a few places
    for i, s in enumerate(sigmas):
        raw[torch.arange(i, K, 97), 3] = s
    return raw, z, offs


LENGTHS = [0, 1, 63, 64, 65, 1024, 0, 300, 7]


@pytest.mark.parametrize("white", [False, True])
def test_packed_composite_forward_matches_the_reference(white):
    from nerf_meets_mlx_amd.rendering import render
    raw, z, offs = _packed(LENGTHS, 1)
    step = M.step_world(1024, 1.5)
    rgb, acc, depth = render.composite_packed(raw.to(DEV), z.to(DEV), offs.to(DEV), len(LENGTHS), step, white)
    w_rgb, w_acc, w_depth = M.composite(raw.double(), z.double(), offs, step, white)
    for nm, a, b in (("rgb", rgb, w_rgb), ("acc", acc, w_acc), ("depth", depth, w_depth)):
        a = a.cpu().double()
        assert bool(torch.isfinite(a).all()), nm
        scale = float(b.abs().max()) + 1e-6
        assert float((a - b).abs().max()) < 2e-4 * scale, nm
    assert float(acc[0]) == 0.0 and float(depth[0]) == 0.0 and rgb[0].tolist() == ([1.0] * 3 if white else [0.0] * 3)
    # a NaN in one ray's raw: that ray NaN, its neighbours bit-identical
    raw_n = raw.clone()
    raw_n[int(offs[3]) + 10, 3] = float("nan")
    rgb_n, acc_n, depth_n = render.composite_packed(raw_n.to(DEV), z.to(DEV), offs.to(DEV), len(LENGTHS), step, white)
    assert bool(torch.isnan(rgb_n[3]).all()) and bool(torch.isnan(acc_n[3])) and bool(torch.isnan(depth_n[3]))
    keep = [b for b in range(len(LENGTHS)) if b != 3]
    assert bits_equal(rgb_n[keep], rgb[keep]) and bits_equal(acc_n[keep], acc[keep])


@pytest.mark.parametrize("white", [False, True])
def test_packed_mse_backward_matches_float64_autograd(white):
    from nerf_meets_mlx_amd.rendering import render
    raw, z, offs = _packed(LENGTHS, 2, sigmas=(-100.0, 0.0, 20.0, 1e30))
    B = len(LENGTHS)
    target = torch.rand(B, 3, generator=torch.Generator().manual_seed(3))
    step = M.step_world(1024, 1.5)
    loss, d_raw, rgb = render.composite_packed_mse_backward(raw.to(DEV), offs.to(DEV), B, step, target.to(DEV), white, need_rgb=True)
    w_loss, w_d = M.mse_backward(raw, offs, step, target, white)
    assert bool(torch.isfinite(d_raw).all()) and bool(torch.isfinite(loss).all())
    assert abs(float(loss) - float(w_loss)) <= 1e-5 * float(w_loss)
    w_rgb, _, _ = M.composite(raw.double(), z.double(), offs, step, white)
    assert float((rgb.cpu().double() - w_rgb).abs().max()) < 2e-4
    got = d_raw.cpu().double()
    np.testing.assert_allclose(got.numpy(), w_d.numpy(), rtol=2e-3, atol=2e-4 * float(w_d.abs().max()))
    # bit-reproducible
    _, d2, _ = render.composite_packed_mse_backward(raw.to(DEV), offs.to(DEV), B, step, target.to(DEV), white)
    assert bits_equal(d2, d_raw)
    # NaN in one ray: only that ray's gradient is NaN
    raw_n = raw.clone()
    raw_n[int(offs[5]) + 3, 3] = float("nan")
    _, dn, _ = render.composite_packed_mse_backward(raw_n.to(DEV), offs.to(DEV), B, step, target.to(DEV), white)
    seg = slice(int(offs[5]), int(offs[6]))
    assert bool(torch.isnan(dn[seg]).any())
    other = torch.ones(raw.shape[0], dtype=torch.bool)
    other[seg] = False
    assert bits_equal(dn[other.to(DEV)], d_raw[other.to(DEV)])


# ------------------------------------------------------------------------------------------------ 4: merge
def test_exp_merge_matches_the_reference_and_relu_merge_is_unchanged():
    from nerf_meets_mlx_amd import _native as N
    from nerf_meets_mlx_amd.engine.occupancy import DECAY, EXP, RELU, RES
    gen = torch.Generator(device=DEV).manual_seed(4)
    n = RES ** 3
    dens = torch.rand(n, device=DEV, generator=gen) * 3.0
    raw = torch.randn(n, 4, device=DEV, generator=gen) * 2.0
    raw[::9973, 3] = float("nan")
    raw[::10007, 3] = float("-inf")
    raw[::10009, 3] = 100.0
    a = dens.clone()
    N.check(N.lib().nerf_occ_merge_ex(N.ptr(a), N.ptr(raw), n, DECAY, EXP, N.stream()))
    d = dens * torch.tensor(DECAY, dtype=torch.float32, device=DEV)
    s = raw[:, 3]
    r = torch.where(torch.isnan(s), torch.zeros_like(s), torch.exp(s))
    want = torch.where(r > d, r, d)
    ulp = (a.view(torch.int32).long() - want.view(torch.int32).long()).abs()
    assert int(ulp.max()) <= 1, int(ulp.max())                 # device expf vs torch's exp: at most one ulp
    assert bool(torch.isfinite(a[9973::9973]).all())          # NaN counts as 0 (index 0 is also one of the exp(100) = inf)
    b, c = dens.clone(), dens.clone()
    N.check(N.lib().nerf_occ_merge(N.ptr(b), N.ptr(raw), n, DECAY, N.stream()))
    N.check(N.lib().nerf_occ_merge_ex(N.ptr(c), N.ptr(raw), n, DECAY, RELU, N.stream()))
    assert bits_equal(b, O.merge(dens, raw[:, 3])) and bits_equal(c, b)


# ------------------------------------------------------------------------------------------------ 5: trainer
def _trainers(hw, views, log2_t, seed, n_rand=256, arms=("march", "march", "off")):
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    imgs, poses, rposes, hwf, K = synthetic.make_dataset(hw, hw, views + 1, seed=0, device=DEV)
    out = [NGPTrainer(imgs[:-1], poses[:-1], K, N_rand=n_rand, n_depth_samples=64, seed=seed, device=DEV,
                      log2_hashmap_size=log2_t, occupancy_grid=(arm == "march"), march_steps=1024 if arm == "march" else None)
           for arm in arms]
    return out, imgs[-1], poses[-1]


def _state(tr):
    f = tr.field
    return [f.mlp.params.clone(), f.enc.tables.clone()] + [t.clone() for k in ("mlp", "tables") for t in tr.opt.state[k]]


def test_trainer_march_is_reproducible_samples_fewer_after_warmup_and_learns():
    """hw 48, 2^14-entry tables, seed 4, 256 rays per step, 600 iterations, march_steps 1024.  Two march runs are bit-identical
    (parameters, tables, Adam moments, grid); after the warm-up the march keeps fewer samples per ray than before it; the
    held-out frame beats the all-white frame.  Measured on an MI355X: 557 samples per ray before the warm-up, 136 over the last
    100 steps; held-out PSNR 16.19 dB (march) against 10.76 dB (grid-free, 64 samples) and 10.13 dB (all-white frame).  The bars
    keep margin: > all-white + 3 dB, and no worse than the grid-free arm."""
    from nerf_meets_mlx_amd.engine.occupancy import WARMUP
    (a, b, off), gt, pose = _trainers(48, 8, 14, 4)
    pre, post = [], []
    for it in range(600):
        la = a.train_step()["loss_coarse"]
        b.train_step()
        off.train_step()
        (pre if it < WARMUP else post).append(a.last_march[1] / 256.0)
    assert np.isfinite(float(la))
    for x, y in zip(_state(a), _state(b)):
        assert bits_equal(x, y)
    assert bits_equal(a.grid.density, b.grid.density) and bits_equal(a.grid.bits, b.grid.bits)
    spr_pre, spr_post = float(np.mean(pre)), float(np.mean(post[-100:]))
    p_march, p_off = a.psnr(pose[:3, :4].numpy(), gt), off.psnr(pose[:3, :4].numpy(), gt)
    p_white = float(-10.0 * torch.log10(((1.0 - gt.double().to(DEV)) ** 2).mean()))
    print(f"\nmarch trainer hw48: samples/ray pre-warmup {spr_pre:.1f} post {spr_post:.1f}; held-out PSNR march {p_march:.2f} "
          f"grid-free {p_off:.2f} all-white {p_white:.2f}")
    assert spr_post < spr_pre
    assert p_march > p_white + 3.0, (p_march, p_white)
    assert p_march > p_off, (p_march, p_off)


# ------------------------------------------------------------------------------------------------ 6: checkpoint
def test_march_checkpoint_resume_is_bit_identical(tmp_path):
    from nerf_meets_mlx_amd.engine.occupancy import WARMUP
    (a,), _, _ = _trainers(32, 4, 14, 4, arms=("march",))
    N_ = 2 * WARMUP + 68                                         # the save (290) lies after the warm-up, between two updates
    for _ in range(N_ // 2):
        a.train_step()
    path = a.save(str(tmp_path / "ckpt"))
    for _ in range(N_ - N_ // 2):
        a.train_step()
    (b,), _, _ = _trainers(32, 4, 14, 9, arms=("march",))
    assert b.load(path) == N_ // 2
    for _ in range(N_ - N_ // 2):
        b.train_step()
    for x, y in zip(_state(b), _state(a)):
        assert bits_equal(x, y)
    assert bits_equal(b.grid.density, a.grid.density) and bits_equal(b.grid.bits, a.grid.bits)


# ------------------------------------------------------------------------------------------------ 7: two ranks
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _march_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    from nerf_meets_mlx_amd import parallel
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    torch.cuda.set_device(0)
    parallel.init_from_env(backend="gloo")
    res = []
    try:
        imgs, poses, _, _, K = synthetic.make_dataset(16, 16, 3, seed=0, device="cuda")
        tr = NGPTrainer(imgs, poses, K, N_rand=64, n_depth_samples=64, seed=4, device="cuda", log2_hashmap_size=14,
                        occupancy_grid=True, march_steps=256)
        for it in range(4):
            rays, target = tr.sample_batch()
            if rank == 1 and it == 2:                            # rank 1 marches nothing at this step: K = 0 there only
                rays = rays.clone()
                rays[:, 0:3] = 10.0
                rays[:, 3:6] = 1.0
            tr.train_step(rays, target)
            ks = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
            dist.all_gather(ks, torch.tensor([tr.last_march[1]], dtype=torch.int64))
            tabs = [torch.zeros_like(tr.field.enc.tables) for _ in range(world)]
            dist.all_gather(tabs, tr.field.enc.tables)
            mlps = [torch.zeros_like(tr.field.mlp.params) for _ in range(world)]
            dist.all_gather(mlps, tr.field.mlp.params)
            res.append(([int(k) for k in ks], torch.equal(tabs[0], tabs[1]) and torch.equal(mlps[0], mlps[1])))
        q.put((rank, res, None))
    except Exception as e:                                       # report, do not hang the other rank's queue read
        q.put((rank, res, repr(e)))
    dist.destroy_process_group()


def test_two_ranks_with_different_sample_counts_stay_identical():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_march_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = [q.get(timeout=280) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, res, err in out:
        assert err is None, (rank, err)
        assert len(res) == 4
        for ks, same in res:
            assert same, (rank, ks)
        assert res[2][0][1] == 0 and res[2][0][0] > 0            # rank 1 had K = 0 while rank 0 had samples
        assert res[0][0][0] != res[0][0][1]
