"""Background colour and RGBA training, host side (no GPU): the float64 reference of tests/_background_ref.py against the existing
white references, the adjoint of acc the kernels use, the teacher's RGBA frames, the argument checks of NGPTrainer / render_rays and
of the C entry points (all made before any device work)."""
import ctypes as C

import pytest
import torch

from tests import _background_ref as R
from tests import _distortion_ref as D
from tests import _ert_ref as E
from tests import _march_ref as M

S = 64
STEP = M.step_world(S, 1.5)
LENGTHS = [0, 1, 2, 63, 64, 65, 0, 130, 7]


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    B = len(LENGTHS)
    offs = torch.zeros(B + 1, dtype=torch.int64)
    offs[1:] = torch.cumsum(torch.tensor(LENGTHS), 0)
    K = int(offs[-1])
    raw = torch.rand(K, 4, generator=g)
    raw[:, 3] = torch.randn(K, generator=g) * 2.0 + 1.0
    z = torch.sort(torch.rand(K, generator=g) * 4 + 2).values
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * (0.5 + 1.5 * torch.rand(B, 1, generator=g))
    rays = torch.cat([torch.randn(B, 3, generator=g), d, torch.tensor([[2.0, 6.0]]).expand(B, 2),
                      torch.nn.functional.normalize(d, dim=-1)], 1).float().contiguous()
    rgba = torch.rand(B, 4, generator=g)
    rgba[0, 3], rgba[1, 3] = 0.0, 1.0
    bg = torch.rand(B, 3, generator=g)
    return raw, z, offs, rays, rgba, bg


def test_with_a_white_background_the_reference_is_the_existing_white_reference():
    raw, z, offs, rays, rgba, _ = _batch(1)
    B = len(LENGTHS)
    one = torch.ones(B, 3)
    for bg in (one, torch.ones(3)):
        rgb, acc, depth = R.composite(raw.double(), z.double(), offs, STEP, bg)
        w_rgb, w_acc, w_depth = M.composite(raw.double(), z.double(), offs, STEP, True)
        assert torch.equal(rgb, w_rgb) and torch.equal(acc, w_acc) and torch.equal(depth, w_depth)
    t = R.target(rgba.double(), one)
    assert torch.equal(t, rgba[:, :3].double() * rgba[:, 3:].double() + (1.0 - rgba[:, 3:].double()))
    mse, _, d_raw, rgb = R.objective_backward(raw, z, offs, rays, STEP, S, rgba, one)
    w_mse, w_d = M.mse_backward(raw, offs, STEP, t, True)
    assert torch.equal(mse, w_mse) and torch.equal(d_raw, w_d)
    mse, dist, d_raw, rgb = R.objective_backward(raw, z, offs, rays, STEP, S, rgba, one, 0.5)
    w_mse, w_dist, w_d, w_rgb = D.objective_backward(raw, z, offs, rays, STEP, S, t, True, 0.5)
    assert torch.equal(mse, w_mse) and torch.equal(dist, w_dist) and torch.equal(d_raw, w_d) and torch.equal(rgb, w_rgb)
    f = R.fold(raw, z, offs, STEP, 1e-2, one)
    w_f = E.fold(raw, z, offs, STEP, 1e-2, True)
    assert all(torch.equal(a, b) for a, b in zip(f, w_f))
    # an opaque target is the image's colour, whatever is behind it; a transparent one is the background
    bg = torch.rand(B, 3, generator=torch.Generator().manual_seed(2))
    t = R.target(rgba, bg)
    assert torch.equal(t[1], rgba[1, :3]) and torch.equal(t[0], bg[0])
    # over black the render is the premultiplied colour
    c, _, _ = M.composite(raw.double(), z.double(), offs, STEP, False)
    assert torch.equal(R.composite(raw.double(), z.double(), offs, STEP, torch.zeros(3))[0], c)


def test_the_adjoint_of_acc_matches_autograd():
    """gacc = -((g_r bg_r + g_g bg_g) + g_b bg_b), g_c = 2 (rgb_c - t_c) / (3 B): the one adjoint term the background changes."""
    raw, z, offs, rays, rgba, bg = _batch(3)
    B = len(LENGTHS)
    g, gacc = R.acc_adjoint(raw, z, offs, STEP, rgba, bg)
    rgb, _, _ = R.composite(raw.double(), z.double(), offs, STEP, bg)
    want_g = 2.0 * (rgb - R.target(rgba.double(), bg.double())) / (3 * B)
    b64 = bg.double()
    want_gacc = -((want_g[:, 0] * b64[:, 0] + want_g[:, 1] * b64[:, 1]) + want_g[:, 2] * b64[:, 2])
    assert float(want_gacc.abs().max()) > 1e-3
    torch.testing.assert_close(g, want_g, rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(gacc, want_gacc, rtol=1e-12, atol=1e-15)
    # and the whole chain: d_raw of the reference through that adjoint is autograd's
    _, _, d_raw, _ = R.objective_backward(raw, z, offs, rays, STEP, S, rgba, bg)
    r = raw.double().requires_grad_(True)
    c, acc, _ = M.composite(r, z.double(), offs, STEP, False)
    ((c * want_g).sum() + (acc * want_gacc).sum()).backward()
    torch.testing.assert_close(r.grad, d_raw, rtol=1e-10, atol=1e-14)


def test_synthetic_rgba_frames_fold_to_the_white_frames():
    """hw 48, all 9 views: rgb a + (1 - a) is the white frame within 1e-6 (a divide and a multiply: a few float32 ulps of values
    <= 1); the default call is untouched; alpha is in [0, 1] and colour is 0 where alpha is."""
    from nerf_meets_mlx_amd.dataset import synthetic
    white, poses, _, _, _ = synthetic.make_dataset(48, 48, 9, seed=0)
    rgba, poses4, _, _, _ = synthetic.make_dataset(48, 48, 9, seed=0, rgba=True)
    assert tuple(white.shape) == (9, 48, 48, 3) and tuple(rgba.shape) == (9, 48, 48, 4) and torch.equal(poses, poses4)
    assert white.dtype == rgba.dtype == torch.float32
    a = rgba[..., 3:]
    err = float((rgba[..., :3] * a + (1.0 - a) - white).abs().max())
    print(f"\nsynthetic RGBA hw48 x 9: max |rgb a + (1 - a) - white| = {err:.2e}; alpha in [{float(a.min()):.3f}, {float(a.max()):.6f}], "
          f"{float((a == 0).float().mean()):.3f} of the pixels empty")
    assert err <= 1e-6
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0 + 1e-6
    assert float((a == 0).float().mean()) > 0.1 and float((a > 0.99).float().mean()) > 0.1
    assert float(rgba[..., :3][(a == 0).expand(-1, -1, -1, 3)].abs().max()) == 0.0
    assert torch.equal(synthetic.render_gt(48, 48, poses[0]), white[0])
    assert torch.equal(synthetic.render_gt(48, 48, poses[0], rgba=True), rgba[0])


def test_trainer_and_renderer_check_their_arguments():
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    rgb3, rgba4 = torch.zeros(2, 4, 4, 3), torch.zeros(2, 4, 4, 4)
    march = dict(occupancy_grid=True, march_steps=64)
    with pytest.raises(ValueError, match="march_steps"):         # random_background without the march
        NGPTrainer(rgba4, None, None, device="cpu", random_background=True)
    with pytest.raises(ValueError, match="march_steps"):
        NGPTrainer(rgba4, None, None, device="cpu", occupancy_grid=True, random_background=True)
    with pytest.raises(ValueError, match="RGBA"):                # ... with 3-channel images
        NGPTrainer(rgb3, None, None, device="cpu", random_background=True, **march)
    with pytest.raises(ValueError, match="post_load_blender_data"):      # RGBA images without it
        NGPTrainer(rgba4, None, None, device="cpu", **march)
    with pytest.raises(ValueError, match="post_load_blender_data"):
        NGPTrainer(rgba4, None, None, device="cpu")
    with pytest.raises(ValueError, match="distortion_weight"):   # the other checks still run
        NGPTrainer(rgba4, None, None, device="cpu", random_background=True, distortion_weight=0.0, **march)
    rays = torch.zeros(5, 11)
    tr = NGPTrainer.__new__(NGPTrainer)                          # the checks come before any device work: no field needed
    tr.march_steps, tr.random_background = None, False
    for bg in ((0.0, 0.0, 0.0), torch.zeros(5, 3)):
        with pytest.raises(ValueError, match="march_steps"):     # the 64-sample modes
            tr.render_rays(rays, background=bg)
        with pytest.raises(ValueError, match="march"):
            Trainer.__new__(Trainer).render_rays(rays, background=bg)
    tr.march_steps = 64
    for bg in ((0.0, 0.0), torch.zeros(4, 3), torch.zeros(5, 4), torch.zeros(2, 5, 3)):
        with pytest.raises(ValueError, match="background"):
            tr.render_rays(rays, background=bg)
    with pytest.raises(ValueError, match="random_background"):
        tr.train_step(rays, torch.zeros(5, 4), background=torch.zeros(5, 3))


def test_background_entry_points_check_their_arguments():
    from nerf_meets_mlx_amd import _native as N
    lib = N.lib()
    p, odd = C.c_void_p(16), C.c_void_p(20)
    OK, E_NULL, E_SHAPE = 0, -1, -2
    fwd, fwd_d = lib.nerf_composite_packed_forward_bg, lib.nerf_composite_packed_distortion_bg
    bwd, bwd_d = lib.nerf_composite_packed_mse_backward_bg, lib.nerf_composite_packed_mse_dist_backward_bg
    fin, smp = lib.nerf_ert_finish_bg, lib.nerf_sample_batch_rgba
    # (raw, z, offsets, B, K, step_world, bg, bg_stride, rgb, acc, depth, stream)
    for stride in (1, 2, 4, -3):
        assert fwd(p, p, p, 4, 8, 0.01, p, stride, p, p, p, None) == E_SHAPE
    assert fwd(p, p, p, 4, 8, 0.0, p, 3, p, p, p, None) == E_SHAPE
    assert fwd(p, p, p, -1, 8, 0.01, p, 3, p, p, p, None) == E_SHAPE
    assert fwd(odd, p, p, 4, 8, 0.01, p, 0, p, p, p, None) == E_SHAPE
    assert fwd(None, None, None, 0, 0, 0.01, None, 0, None, None, None, None) == OK
    assert fwd(None, None, None, 0, 0, 0.01, None, 1, None, None, None, None) == E_SHAPE           # checked before B = 0
    for i in (0, 1, 2, 6, 8):                                    # raw, z, offsets, bg, rgb
        a = [p, p, p, 4, 8, 0.01, p, 3, p, p, p, None]
        a[i] = None
        assert fwd(*a) == E_NULL, i
    # (raw, z, offsets, rays, B, K, step_world, march_steps, bg, bg_stride, rgb, acc, depth, dist, stream)
    assert fwd_d(p, p, p, p, 4, 8, 0.01, 0, p, 3, p, p, p, p, None) == E_SHAPE
    assert fwd_d(p, p, p, p, 4, 8, 0.01, 64, p, 1, p, p, p, p, None) == E_SHAPE
    assert fwd_d(odd, p, p, p, 4, 8, 0.01, 64, p, 3, p, p, p, p, None) == E_SHAPE
    assert fwd_d(None, None, None, None, 0, 0, 0.01, 64, None, 3, None, None, None, None, None) == OK
    for i in (0, 1, 2, 3, 8, 10, 13):                            # raw, z, offsets, rays, bg, rgb, dist
        a = [p, p, p, p, 4, 8, 0.01, 64, p, 3, p, p, p, p, None]
        a[i] = None
        assert fwd_d(*a) == E_NULL, i
    # (raw, offsets, B, K, step_world, target_rgba, bg, grad_scale, loss, rgb, d_raw, stream)
    assert bwd(p, p, 4, 8, 0.0, p, p, 1.0, p, p, p, None) == E_SHAPE
    assert bwd(odd, p, 4, 8, 0.01, p, p, 1.0, p, p, p, None) == E_SHAPE
    assert bwd(p, p, 4, 8, 0.01, odd, p, 1.0, p, p, p, None) == E_SHAPE
    assert bwd(p, p, 4, 8, 0.01, p, p, 1.0, p, p, odd, None) == E_SHAPE
    assert bwd(None, None, 0, 0, 0.01, None, None, 1.0, None, None, None, None) == OK
    for i in (0, 1, 5, 6, 10):                                   # raw, offsets, target_rgba, bg, d_raw
        a = [p, p, 4, 8, 0.01, p, p, 1.0, p, p, p, None]
        a[i] = None
        assert bwd(*a) == E_NULL, i
    # (raw, z, offsets, rays, B, K, step_world, march_steps, target_rgba, bg, grad_scale, dist_weight, loss, dist, rgb, d_raw, stream)
    assert bwd_d(p, p, p, p, 4, 8, 0.01, 2048, p, p, 1.0, 0.01, p, p, p, p, None) == E_SHAPE
    for w in (-0.01, float("nan"), float("inf")):
        assert bwd_d(p, p, p, p, 4, 8, 0.01, 64, p, p, 1.0, w, p, p, p, p, None) == E_SHAPE, w
    assert bwd_d(p, p, p, p, 4, 8, 0.01, 64, odd, p, 1.0, 0.01, p, p, p, p, None) == E_SHAPE
    assert bwd_d(None, None, None, None, 0, 0, 0.01, 64, None, None, 1.0, 0.01, None, None, None, None, None) == OK
    for i in (0, 1, 2, 3, 8, 9, 15):                             # raw, z, offsets, rays, target_rgba, bg, d_raw
        a = [p, p, p, p, 4, 8, 0.01, 64, p, p, 1.0, 0.01, p, p, p, p, None]
        a[i] = None
        assert bwd_d(*a) == E_NULL, i
    # (istate, fstate, B, bg, bg_stride, rgb, acc, depth, samples, stream)
    assert fin(p, p, 4, p, 2, p, p, p, p, None) == E_SHAPE
    assert fin(p, p, -1, p, 3, p, p, p, p, None) == E_SHAPE
    assert fin(None, None, 0, None, 0, None, None, None, None, None) == OK
    for i in (0, 1, 3, 5):                                       # istate, fstate, bg, rgb
        a = [p, p, 4, p, 3, p, p, p, p, None]
        a[i] = None
        assert fin(*a) == E_NULL, i
    # (n, H, W, seed, offset, K, c2w, near, far, image, rays, target, pixel_idx, stream)
    Kc, cc = (C.c_double * 9)(), (C.c_float * 12)()
    assert smp(4, 0, 8, 1, 0, Kc, cc, 2.0, 6.0, p, p, p, None, None) == E_SHAPE
    assert smp(65, 8, 8, 1, 0, Kc, cc, 2.0, 6.0, p, p, p, None, None) == E_SHAPE
    assert smp(4, 8, 8, 1, 0, Kc, cc, 2.0, 6.0, odd, p, p, None, None) == E_SHAPE
    assert smp(4, 8, 8, 1, 0, Kc, cc, 2.0, 6.0, p, p, odd, None, None) == E_SHAPE
    assert smp(0, 8, 8, 1, 0, None, None, 2.0, 6.0, None, None, None, None, None) == OK
    for i in (9, 10, 11):                                        # image, rays, target
        a = [4, 8, 8, 1, 0, Kc, cc, 2.0, 6.0, p, p, p, None, None]
        a[i] = None
        assert smp(*a) == E_NULL, i
    assert lib.nerf_abi_version() == 3
