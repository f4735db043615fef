"""Distortion regulariser on the GPU (csrc/composite_packed.hip nerf_composite_packed_distortion / _mse_dist_backward,
NGPTrainer(distortion_weight=...)) against the float64 reference of tests/_distortion_ref.py: the forward dist and the training
form's loss, dist_out, rgb and d_raw over mixed segment lengths, the regulariser's gradient alone, poisoned buffers, the edge cases
of include/nerf_hip.h "distortion regulariser", bit-reproducibility, and two trainers side by side.

Tolerances are packed compositing's (tests/test_gpu_march.py): loss 1e-5 relative, rgb 2e-4, d_raw rtol 2e-3 with atol 2e-4 of
its largest magnitude; dist per ray 1e-5 relative plus an absolute floor of 1e-7 for near-empty rays."""
import numpy as np
import pytest
import torch

from tests import _distortion_ref as D
from tests import _march_ref as M
from tests._poison import bits_equal, sentinel_, unwritten
from tests.test_gpu_march import _packed

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 1024
STEP = M.step_world(S, 1.5)
LENGTHS = [0, 1, 2, 63, 64, 65, 0, 300, 1024, 0, 7]
SIGMAS_FWD = (-100.0, 0.0, 20.0, 100.0, 1e30)
SIGMAS_BWD = (-100.0, 0.0, 20.0, 1e30)
SHIFT = {"thin": -4.0, "mixed": 0.0, "saturated": 5.0}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _batch(seed, sigmas, density, lengths=LENGTHS):
    """(raw [K, 4], z [K], offsets [B + 1], rays [B, 11]) on the CPU: test_gpu_march._packed's samples with the ordinary densities
    shifted to thin / saturated rays (the special ones stay), and rays whose d has a length between 0.5 and 2."""
    raw, z, offs = _packed(lengths, seed, sigmas=sigmas)
    special = torch.zeros(raw.shape[0], dtype=torch.bool)
    for s in sigmas:
        special |= raw[:, 3] == s
    raw[~special, 3] += SHIFT[density]
    g = torch.Generator().manual_seed(seed + 1000)
    B = len(lengths)
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * (0.5 + 1.5 * torch.rand(B, 1, generator=g))
    o = torch.randn(B, 3, generator=g)
    nf = torch.tensor([[2.0, 6.0]]).expand(B, 2)
    rays = torch.cat([o, d, nf, torch.nn.functional.normalize(d, dim=-1)], 1).float().contiguous()
    return raw, z, offs, rays


def _dev(*ts):
    return [t.to(DEV) for t in ts]


def _close_dist(got, want, what):
    got, want = got.cpu().double().reshape(-1), want.double().reshape(-1)
    err = (got - want).abs()
    print(f"\n{what}: dist max {float(want.max()):.3e}, worst error {float((err / (want.abs() + 1e-30)).max()):.1e} relative, "
          f"{float(err.max()):.1e} absolute")
    assert bool(torch.isfinite(got).all()), what
    assert bool((err <= 1e-5 * want.abs() + 1e-7).all()), (what, err.tolist(), want.tolist())


# ------------------------------------------------------------------------------------------------ 1: forward
@pytest.mark.parametrize("density", ["thin", "mixed", "saturated"])
@pytest.mark.parametrize("white", [False, True])
def test_forward_dist_matches_the_reference(white, density):
    from nerf_meets_mlx_amd.rendering import render
    raw, z, offs, rays = _batch(1, SIGMAS_FWD, density)
    B = len(LENGTHS)
    rgb, acc, depth, dist = render.composite_packed_distortion(*_dev(raw, z, offs, rays), STEP, S, white)
    w_rgb, w_acc, w_depth = M.composite(raw.double(), z.double(), offs, STEP, white)
    for nm, a, b in (("rgb", rgb, w_rgb), ("acc", acc, w_acc), ("depth", depth, w_depth)):
        a = a.cpu().double()
        assert bool(torch.isfinite(a).all()), nm
        assert float((a - b).abs().max()) < 2e-4 * (float(b.abs().max()) + 1e-6), nm
    _close_dist(dist, D.losses(raw.double(), z, offs, rays, STEP, S), f"forward white={white} {density}")
    for b in (0, 6, 9):                                          # rays without samples
        assert float(dist[b]) == 0.0 and float(acc[b]) == 0.0
    assert float(dist.min()) >= 0.0
    # the other outputs are the packed forward's, bit for bit (the same operations)
    rgb0, acc0, depth0 = render.composite_packed(*_dev(raw, z, offs), B, STEP, white)
    assert bits_equal(rgb, rgb0) and bits_equal(acc, acc0) and bits_equal(depth, depth0)


# ------------------------------------------------------------------------------------------------ 2: training form
@pytest.mark.parametrize("density", ["thin", "mixed", "saturated"])
@pytest.mark.parametrize("white", [False, True])
def test_training_form_matches_float64_autograd(white, density):
    from nerf_meets_mlx_amd.rendering import render
    raw, z, offs, rays = _batch(2, SIGMAS_BWD, density)
    B = len(LENGTHS)
    target = torch.rand(B, 3, generator=torch.Generator().manual_seed(3))
    lam = 10.0                                                   # large, so that both terms weigh in d_raw
    loss, dist, d_raw, rgb = render.composite_packed_mse_dist_backward(*_dev(raw, z, offs, rays), STEP, S, target.to(DEV), lam, white,
                                                                       need_rgb=True)
    w_loss, w_dist, w_d, w_rgb = D.objective_backward(raw, z, offs, rays, STEP, S, target, white, lam)
    assert bool(torch.isfinite(d_raw).all()) and bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dist).all())
    print(f"\ntraining white={white} {density}: loss {float(loss):.6e} / {float(w_loss):.6e}, dist {float(dist):.6e} / {float(w_dist):.6e}")
    assert abs(float(loss) - float(w_loss)) <= 1e-5 * float(w_loss)
    assert abs(float(dist) - float(w_dist)) <= 1e-5 * float(w_dist) + 1e-7
    assert float((rgb.cpu().double() - w_rgb).abs().max()) < 2e-4
    np.testing.assert_allclose(d_raw.cpu().double().numpy(), w_d.numpy(), rtol=2e-3, atol=2e-4 * float(w_d.abs().max()))
    # weight 0 is the packed MSE backward (G + 0 = G; a zero may change its sign), and loss / rgb do not depend on the weight
    loss0, dist0, d0, rgb0 = render.composite_packed_mse_dist_backward(*_dev(raw, z, offs, rays), STEP, S, target.to(DEV), 0.0, white,
                                                                       need_rgb=True)
    _, d_plain, rgb_plain = render.composite_packed_mse_backward(*_dev(raw, offs), B, STEP, target.to(DEV), white, need_rgb=True)
    assert torch.equal(d0, d_plain) and bits_equal(rgb0, rgb_plain) and bits_equal(rgb, rgb_plain)
    assert abs(float(dist0) - float(dist)) <= 1e-6 * float(dist)


@pytest.mark.parametrize("white", [False, True])
def test_with_the_rendered_rgb_as_target_the_gradient_is_the_regularisers_alone(white):
    from nerf_meets_mlx_amd.rendering import render
    raw, z, offs, rays = _batch(4, SIGMAS_BWD, "mixed")
    lam = 1e-2
    rgb, _, _, _ = render.composite_packed_distortion(*_dev(raw, z, offs, rays), STEP, S, white)
    loss, dist, d_raw, _ = render.composite_packed_mse_dist_backward(*_dev(raw, z, offs, rays), STEP, S, rgb, lam, white)
    assert float(loss) == 0.0 and float(dist) > 0.0
    assert float(d_raw[:, :3].abs().max()) == 0.0               # the colour columns do not see the new term
    assert float(d_raw[:, 3].abs().max()) > 0.0
    w_rgb, _, _ = M.composite(raw.double(), z.double(), offs, STEP, white)
    _, _, w_d, _ = D.objective_backward(raw, z, offs, rays, STEP, S, w_rgb, white, lam)
    np.testing.assert_allclose(d_raw.cpu().double().numpy(), w_d.numpy(), rtol=2e-3, atol=2e-4 * float(w_d.abs().max()))


# ------------------------------------------------------------------------------------------------ 3: poisoned buffers
def test_every_output_is_written_and_nothing_outside():
    from nerf_meets_mlx_amd import _native as N
    raw, z, offs, rays = _dev(*_batch(5, SIGMAS_BWD, "mixed"))
    B, K, PAD = len(LENGTHS), raw.shape[0], 8
    target = torch.rand(B, 3, device=DEV)

    def guarded(rows, cols):
        full = sentinel_(torch.empty(rows + 2 * PAD, cols, dtype=torch.float32, device=DEV))
        return full, full[PAD:PAD + rows]

    def check(full, inner, what):
        assert unwritten(inner) == 0, what
        assert unwritten(full) == 2 * PAD * full.shape[1], what

    bufs = {k: guarded(r, c) for k, r, c in (("rgb", B, 3), ("acc", B, 1), ("depth", B, 1), ("dist", B, 1))}
    N.check(N.lib().nerf_composite_packed_distortion(N.ptr(raw), N.ptr(z), N.ptr(offs), N.ptr(rays), B, K, STEP, S, 1,
                                                     N.ptr(bufs["rgb"][1]), N.ptr(bufs["acc"][1]), N.ptr(bufs["depth"][1]),
                                                     N.ptr(bufs["dist"][1]), N.stream()))
    for k, (full, inner) in bufs.items():
        check(full, inner, "forward " + k)
    d_full, d_in = guarded(K, 4)
    r_full, r_in = guarded(B, 3)
    loss, dist = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    N.check(N.lib().nerf_composite_packed_mse_dist_backward(N.ptr(raw), N.ptr(z), N.ptr(offs), N.ptr(rays), B, K, STEP, S, 1,
                                                            N.ptr(target), 1.0, 1e-2, N.ptr(loss), N.ptr(dist), N.ptr(r_in),
                                                            N.ptr(d_in), N.stream()))
    check(d_full, d_in, "training d_raw")
    check(r_full, r_in, "training rgb")
    assert float(loss) > 0.0 and float(dist) > 0.0
    # NULL optional outputs: acc, depth; loss, dist_out, rgb
    _, dist_only = guarded(B, 1)
    _, rgb_only = guarded(B, 3)
    N.check(N.lib().nerf_composite_packed_distortion(N.ptr(raw), N.ptr(z), N.ptr(offs), N.ptr(rays), B, K, STEP, S, 1,
                                                     N.ptr(rgb_only), None, None, N.ptr(dist_only), N.stream()))
    assert bits_equal(dist_only, bufs["dist"][1]) and bits_equal(rgb_only, bufs["rgb"][1])
    d2_full, d2_in = guarded(K, 4)
    N.check(N.lib().nerf_composite_packed_mse_dist_backward(N.ptr(raw), N.ptr(z), N.ptr(offs), N.ptr(rays), B, K, STEP, S, 1,
                                                            N.ptr(target), 1.0, 1e-2, None, None, None, N.ptr(d2_in), N.stream()))
    assert bits_equal(d2_in, d_in)
    # no rays, and rays without any sample
    assert N.lib().nerf_composite_packed_distortion(None, None, None, None, 0, 0, STEP, S, 1, None, None, None, None, N.stream()) == 0
    o0 = torch.zeros(B + 1, dtype=torch.int64, device=DEV)
    e_full, e_in = guarded(B, 1)
    N.check(N.lib().nerf_composite_packed_mse_dist_backward(None, None, N.ptr(o0), N.ptr(rays), B, 0, STEP, S, 1, N.ptr(target), 1.0,
                                                            1e-2, N.ptr(loss), N.ptr(dist), None, None, N.stream()))
    N.check(N.lib().nerf_composite_packed_distortion(None, None, N.ptr(o0), N.ptr(rays), B, 0, STEP, S, 1, N.ptr(rgb_only), None, None,
                                                     N.ptr(e_in), N.stream()))
    check(e_full, e_in, "empty dist")
    assert float(e_in.abs().max()) == 0.0 and float(rgb_only.min()) == 1.0


# ------------------------------------------------------------------------------------------------ 4: edge cases
def test_nan_inf_bad_offsets_and_degenerate_directions():
    from nerf_meets_mlx_amd.rendering import render
    raw, z, offs, rays = _batch(6, SIGMAS_BWD, "mixed")
    B, K = len(LENGTHS), raw.shape[0]
    target = torch.rand(B, 3, generator=torch.Generator().manual_seed(8)).to(DEV)
    lam = 0.25

    def run(raw_, z_, offs_, rays_):
        a = _dev(raw_, z_, offs_, rays_)
        _, _, _, dist = render.composite_packed_distortion(*a, STEP, S, True)
        _, mean, d_raw, rgb = render.composite_packed_mse_dist_backward(*a, STEP, S, target, lam, True, need_rgb=True)
        return dist, d_raw, rgb, mean

    dist, d_raw, rgb, mean = run(raw, z, offs, rays)
    assert bool(torch.isfinite(dist).all()) and bool(torch.isfinite(d_raw).all())           # sigma = +inf samples included
    assert int((raw[:, 3] == 1e30).sum()) > 0
    seg = lambda b: slice(int(offs[b]), int(offs[b + 1]))
    rows_of = lambda b: torch.arange(K)[seg(b)]

    def others(bs):
        keep_r = torch.ones(B, dtype=torch.bool)
        keep_k = torch.ones(K, dtype=torch.bool)
        for b in bs:
            keep_r[b] = False
            keep_k[seg(b)] = False
        return keep_r.to(DEV), keep_k.to(DEV)

    # a NaN in one ray's raw / in one ray's z: that ray's dist and d_raw NaN, every other ray bit-identical
    for what, b in (("raw", 7), ("z", 8), ("z", 3)):
        raw_n, z_n = raw.clone(), z.clone()
        if what == "raw":
            raw_n[int(offs[b]) + 3, 3] = float("nan")
        else:
            z_n[int(offs[b]) + 2] = float("nan")
        dist_n, d_n, _, mean_n = run(raw_n, z_n, offs, rays)
        assert bool(torch.isnan(dist_n[b])) and bool(torch.isnan(d_n[seg(b)]).any()) and bool(torch.isnan(mean_n).all()), (what, b)
        kr, kk = others([b])
        assert bits_equal(dist_n[kr], dist[kr]) and bits_equal(d_n[kk], d_raw[kk]), (what, b)
    # bad offsets: rays 4 (ends beyond K) and 5 (decreasing) get NaN outputs, nobody else changes
    offs_b = offs.clone()
    offs_b[5] = K + 10
    dist_b, d_b, rgb_b, _ = run(raw, z, offs_b, rays)
    kr, kk = others([4, 5])
    assert bool(torch.isnan(dist_b[[4, 5]]).all()) and bool(torch.isnan(rgb_b[[4, 5]]).all())
    assert bits_equal(dist_b[kr], dist[kr]) and bits_equal(d_b[kk], d_raw[kk]) and bits_equal(rgb_b[kr], rgb[kr])
    # a zero-length and a non-finite d: dist = 0 and no extra gradient for those rays (the packed MSE backward's rows)
    _, d_plain, _ = render.composite_packed_mse_backward(*_dev(raw, offs), B, STEP, target, True)
    for bad in (0.0, float("nan"), float("inf")):
        rays_z = rays.clone()
        rays_z[7, 3:6] = bad
        rays_z[8, 3:6] = bad
        dist_z, d_z, rgb_z, mean_z = run(raw, z, offs, rays_z)
        assert float(dist_z[7]) == 0.0 and float(dist_z[8]) == 0.0 and bool(torch.isfinite(mean_z).all()), bad
        for b in (7, 8):
            assert torch.equal(d_z[seg(b)], d_plain[seg(b)]), bad
            assert not torch.equal(d_raw[seg(b)], d_plain[seg(b)])
        kr, kk = others([7, 8])
        assert bits_equal(dist_z[kr], dist[kr]) and bits_equal(d_z[kk], d_raw[kk]) and bits_equal(rgb_z, rgb), bad
    assert rows_of(8).numel() == 1024


# ------------------------------------------------------------------------------------------------ 5: reproducibility
def test_bit_reproducible_over_launches_and_under_a_permutation_of_the_rays():
    from nerf_meets_mlx_amd.rendering import render
    raw, z, offs, rays = _batch(7, SIGMAS_BWD, "mixed")
    B = len(LENGTHS)
    target = torch.rand(B, 3, generator=torch.Generator().manual_seed(9))
    lam = 0.1

    def run(raw_, z_, offs_, rays_, target_):
        a = _dev(raw_, z_, offs_, rays_)
        dist = render.composite_packed_distortion(*a, STEP, S, True)[3]
        _, _, d_raw, _ = render.composite_packed_mse_dist_backward(*a, STEP, S, target_.to(DEV), lam, True)
        return dist, d_raw

    dist, d_raw = run(raw, z, offs, rays, target)
    for _ in range(3):
        dist2, d2 = run(raw, z, offs, rays, target)
        assert bits_equal(dist2, dist) and bits_equal(d2, d_raw)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(10))
    segs = [slice(int(offs[b]), int(offs[b + 1])) for b in perm.tolist()]
    raw_p, z_p = torch.cat([raw[s] for s in segs]), torch.cat([z[s] for s in segs])
    offs_p = torch.zeros(B + 1, dtype=torch.int64)
    offs_p[1:] = torch.cumsum(torch.tensor([LENGTHS[b] for b in perm.tolist()]), 0)
    dist_p, d_p = run(raw_p, z_p, offs_p, rays[perm], target[perm])
    assert bits_equal(dist_p, dist[perm.to(DEV)])
    assert bits_equal(d_p, torch.cat([d_raw[s] for s in segs]))


# ------------------------------------------------------------------------------------------------ 6: trainer
def _trainer(imgs, poses, K, weight):
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    return NGPTrainer(imgs[:-1], poses[:-1], K, N_rand=256, n_depth_samples=64, seed=4, device=DEV, log2_hashmap_size=14,
                      occupancy_grid=True, march_steps=1024, distortion_weight=weight)


def _state(tr):
    f = tr.field
    return [f.mlp.params.clone(), f.enc.tables.clone()] + [t.clone() for k in ("mlp", "tables") for t in tr.opt.state[k]]


def test_trainer_with_and_without_the_regulariser():
    """The set-up of test_gpu_march's trainer test (hw 48, 8 views, 2^14-entry tables, seed 4, 256 rays per step, march_steps
    1024, 600 iterations), distortion_weight None and 1e-2 side by side.  (a) the None arm's first 32 steps give bit-identical
    parameters to a second None trainer; (b) two weighted runs are bit-identical; (c) the weighted arm's mean L_b over the held-out
    frame (NGPTrainer.ray_distortion: the forward entry) is strictly below the None arm's; (d) the weighted arm has not collapsed:
    its held-out PSNR beats the all-white frame by at least half of the None arm's margin.  The figures measured on an MI355X are
    in DESIGN.md section 15."""
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.rendering import ray
    imgs, poses, _, _, K = synthetic.make_dataset(48, 48, 9, seed=0, device=DEV)
    gt, pose = imgs[-1], poses[-1]
    none, none2, wa, wb = _trainer(imgs, poses, K, None), _trainer(imgs, poses, K, None), _trainer(imgs, poses, K, 1e-2), \
        _trainer(imgs, poses, K, 1e-2)
    logged = []
    for it in range(600):
        o = none.train_step()
        assert set(o) == {"loss_coarse"}
        ow = wa.train_step()
        assert set(ow) == {"loss_coarse", "loss_distortion"}
        wb.train_step()
        if it < 32:
            none2.train_step()
        if it == 31:
            for x, y in zip(_state(none), _state(none2)):
                assert bits_equal(x, y)                          # (a)
        if it % 100 == 99:
            logged.append((it + 1, float(o["loss_coarse"]), float(ow["loss_coarse"]), float(ow["loss_distortion"])))
    assert all(np.isfinite(v) for row in logged for v in row)
    for x, y in zip(_state(wa), _state(wb)):
        assert bits_equal(x, y)                                  # (b)
    assert bits_equal(wa.grid.density, wb.grid.density) and bits_equal(wa.grid.bits, wb.grid.bits)
    c2w = pose[:3, :4].numpy()
    rays = ray.gen_rays(48, 48, none.K, c2w, 2.0, 6.0, torch.arange(48 * 48, device=DEV, dtype=torch.int64))
    l_none, l_w = float(none.ray_distortion(rays).double().mean()), float(wa.ray_distortion(rays).double().mean())
    p_none, p_w = none.psnr(c2w, gt), wa.psnr(c2w, gt)
    p_white = float(-10.0 * torch.log10(((1.0 - gt.double().to(DEV)) ** 2).mean()))
    aux = wa.render_rays(rays, aux=True)
    aux_none = none.render_rays(rays, aux=True)
    print(f"\ndistortion trainer hw48, 600 it: held-out mean L_b none {l_none:.4e} weighted {l_w:.4e}; PSNR none {p_none:.2f} weighted "
          f"{p_w:.2f} all-white {p_white:.2f}; mean acc none {float(aux_none['acc'].mean()):.3f} weighted {float(aux['acc'].mean()):.3f}; "
          f"samples/ray none {float(aux_none['samples'].float().mean()):.1f} weighted {float(aux['samples'].float().mean()):.1f}; "
          f"(it, mse none, mse weighted, train L) {logged}")
    assert set(aux_none) == {"rgb", "acc", "depth", "samples"} and set(aux) == {"rgb", "acc", "depth", "samples", "distortion"}
    assert bits_equal(aux["distortion"], wa.ray_distortion(rays))
    assert np.isfinite(l_none) and np.isfinite(l_w) and l_w < l_none, (l_w, l_none)               # (c)
    assert p_none > p_white, (p_none, p_white)
    assert p_w - p_white >= 0.5 * (p_none - p_white), (p_w, p_none, p_white)                      # (d)
