"""Background colour and RGBA training on the GPU (csrc/composite_packed.hip nerf_composite_packed_*_bg / nerf_ert_finish_bg,
csrc/rays.hip nerf_sample_batch_rgba, NGPTrainer(random_background=True) and render_rays(background=...)) against the float64
reference of tests/_background_ref.py: forward, training form and training + distortion over mixed segment lengths, the three bit
identities of include/nerf_hip.h "background colour", poisoned buffers, the edge cases, bit-reproducibility, early termination, the
RGBA batch sampler, and a white-background trainer beside a random-background one.

Tolerances are packed compositing's (tests/test_gpu_march.py, tests/test_gpu_distortion.py): loss 1e-5 relative, rgb 2e-4, d_raw
rtol 2e-3 with atol 2e-4 of its largest magnitude; dist 1e-5 relative plus an absolute floor of 1e-7."""
import numpy as np
import pytest
import torch

from tests import _background_ref as R
from tests import _distortion_ref as D
from tests._poison import bits_equal, sentinel_, unwritten
from tests.test_gpu_distortion import LENGTHS, S, SIGMAS_BWD, SIGMAS_FWD, STEP, _batch, _close_dist, _dev
from tests.test_gpu_ert import _Dense, _random_bits
from tests.test_gpu_march import _field, _grid, _rays

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = len(LENGTHS)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _colours(seed):
    """(rgba [B, 4], bg [B, 3]) on the CPU: random, with a = 0 on rays 1 and 7 and a = 1 on rays 2 and 8."""
    g = torch.Generator().manual_seed(seed)
    rgba, bg = torch.rand(B, 4, generator=g), torch.rand(B, 3, generator=g)
    rgba[[1, 7], 3] = 0.0
    rgba[[2, 8], 3] = 1.0
    return rgba, bg


def _close_d_raw(got, want):
    np.testing.assert_allclose(got.cpu().double().numpy(), want.numpy(), rtol=2e-3, atol=2e-4 * float(want.abs().max()))


# ------------------------------------------------------------------------------------------------ 1: against the float64 reference
@pytest.mark.parametrize("density", ["thin", "mixed", "saturated"])
def test_forward_matches_the_reference(density):
    from nerf_meets_mlx_amd.rendering import render
    raw, z, offs, rays = _batch(1, SIGMAS_FWD, density)
    _, bg = _colours(2)
    for colour in (bg, bg[3]):                                   # one colour per ray (stride 3) / one for all rays (stride 0)
        arg = colour.to(DEV) if colour.dim() == 2 else tuple(colour.tolist())
        rgb, acc, depth = render.composite_packed_bg(*_dev(raw, z, offs), B, STEP, arg)
        w_rgb, w_acc, w_depth = R.composite(raw.double(), z.double(), offs, STEP, colour)
        for nm, a, b in (("rgb", rgb, w_rgb), ("acc", acc, w_acc), ("depth", depth, w_depth)):
            a = a.cpu().double()
            assert bool(torch.isfinite(a).all()), nm
            assert float((a - b).abs().max()) < 2e-4 * (float(b.abs().max()) + 1e-6), nm
        for b in (0, 6, 9):                                      # rays without samples: the background itself
            assert float(acc[b]) == 0.0 and torch.equal(rgb[b].cpu(), colour[b] if colour.dim() == 2 else colour)
        rgb_d, acc_d, depth_d, dist = render.composite_packed_distortion_bg(*_dev(raw, z, offs, rays), STEP, S, arg)
        assert bits_equal(rgb_d, rgb) and bits_equal(acc_d, acc) and bits_equal(depth_d, depth)
        _close_dist(dist, D.losses(raw.double(), z, offs, rays, STEP, S), f"forward bg {density}")
        dist0 = render.composite_packed_distortion(*_dev(raw, z, offs, rays), STEP, S, True)[3]
        assert bits_equal(dist, dist0)                           # the background does not enter L_b


@pytest.mark.parametrize("density", ["thin", "mixed", "saturated"])
@pytest.mark.parametrize("lam", [0.0, 10.0])
def test_training_forms_match_float64_autograd(lam, density):
    from nerf_meets_mlx_amd.rendering import render
    raw, z, offs, rays = _batch(2, SIGMAS_BWD, density)
    rgba, bg = _colours(3)
    if lam:
        loss, dist, d_raw, rgb = render.composite_packed_mse_dist_backward_bg(*_dev(raw, z, offs, rays), STEP, S, rgba.to(DEV),
                                                                              bg.to(DEV), lam, need_rgb=True)
    else:
        loss, d_raw, rgb = render.composite_packed_mse_backward_bg(*_dev(raw, offs), B, STEP, rgba.to(DEV), bg.to(DEV), need_rgb=True)
    w_loss, w_dist, w_d, w_rgb = R.objective_backward(raw, z, offs, rays, STEP, S, rgba, bg, lam)
    assert bool(torch.isfinite(d_raw).all()) and bool(torch.isfinite(loss).all())
    print(f"\ntraining bg lam={lam} {density}: loss {float(loss):.6e} / {float(w_loss):.6e}, |d_raw| max {float(w_d.abs().max()):.3e}, "
          f"worst d_raw error {float((d_raw.cpu().double() - w_d).abs().max()):.2e}, rgb error "
          f"{float((rgb.cpu().double() - w_rgb).abs().max()):.2e}")
    assert abs(float(loss) - float(w_loss)) <= 1e-5 * float(w_loss)
    assert float((rgb.cpu().double() - w_rgb).abs().max()) < 2e-4
    _close_d_raw(d_raw, w_d)
    if lam:
        assert abs(float(dist) - float(w_dist)) <= 1e-5 * float(w_dist) + 1e-7
        # weight 0 is the plain background form (G + 0 = G; a zero may change its sign)
        _, _, d0, rgb0 = render.composite_packed_mse_dist_backward_bg(*_dev(raw, z, offs, rays), STEP, S, rgba.to(DEV), bg.to(DEV), 0.0,
                                                                      need_rgb=True)
        _, d_plain, rgb_plain = render.composite_packed_mse_backward_bg(*_dev(raw, offs), B, STEP, rgba.to(DEV), bg.to(DEV),
                                                                        need_rgb=True)
        assert torch.equal(d0, d_plain) and bits_equal(rgb0, rgb_plain) and bits_equal(rgb, rgb_plain)


# ------------------------------------------------------------------------------------------------ 2: the three identities
@pytest.mark.parametrize("density", ["thin", "mixed", "saturated"])
def test_a_white_background_gives_the_bits_of_the_white_kernels(density):
    from nerf_meets_mlx_amd.rendering import render
    raw, z, offs, rays = _dev(*_batch(4, SIGMAS_BWD, density))
    rgba = _colours(5)[0].to(DEV)
    ones = torch.ones(B, 3, device=DEV)
    want = render.composite_packed(raw, z, offs, B, STEP, True)
    want_d = render.composite_packed_distortion(raw, z, offs, rays, STEP, S, True)
    for colour in (ones, (1.0, 1.0, 1.0)):
        assert all(bits_equal(a, b) for a, b in zip(render.composite_packed_bg(raw, z, offs, B, STEP, colour), want))
        assert all(bits_equal(a, b) for a, b in zip(render.composite_packed_distortion_bg(raw, z, offs, rays, STEP, S, colour), want_d))
    a = rgba[:, 3:]
    t = rgba[:, :3] * a + ones * (1.0 - a)                       # float32, one rounding per operation: the kernel's t
    loss, d_raw, rgb = render.composite_packed_mse_backward_bg(raw, offs, B, STEP, rgba, ones, need_rgb=True)
    w_loss, w_d, w_rgb = render.composite_packed_mse_backward(raw, offs, B, STEP, t, True, need_rgb=True)
    assert bits_equal(d_raw, w_d) and bits_equal(rgb, w_rgb)
    assert abs(float(loss) - float(w_loss)) <= 1e-6 * float(w_loss)          # a sum of float atomics
    loss, dist, d_raw, rgb = render.composite_packed_mse_dist_backward_bg(raw, z, offs, rays, STEP, S, rgba, ones, 0.3, need_rgb=True)
    w_loss, w_dist, w_d, w_rgb = render.composite_packed_mse_dist_backward(raw, z, offs, rays, STEP, S, t, 0.3, True, need_rgb=True)
    assert bits_equal(d_raw, w_d) and bits_equal(rgb, w_rgb)
    assert abs(float(loss) - float(w_loss)) <= 1e-6 * float(w_loss) and abs(float(dist) - float(w_dist)) <= 1e-6 * float(w_dist)


def test_an_opaque_target_is_the_images_colour_exactly():
    from nerf_meets_mlx_amd.rendering import render
    raw, z, offs, rays = _dev(*_batch(6, SIGMAS_BWD, "mixed"))
    rgba, bg = (t.to(DEV) for t in _colours(7))
    rgba[:, 3] = 1.0
    ones = torch.ones(B, 3, device=DEV)
    # over white: the white kernel fed rgba[:, :3]
    _, d_raw, rgb = render.composite_packed_mse_backward_bg(raw, offs, B, STEP, rgba, ones, need_rgb=True)
    _, w_d, w_rgb = render.composite_packed_mse_backward(raw, offs, B, STEP, rgba[:, :3].contiguous(), True, need_rgb=True)
    assert bits_equal(d_raw, w_d) and bits_equal(rgb, w_rgb)
    # over any colour: with the rendered rgb as an opaque target every error is exactly zero
    rgb = render.composite_packed_bg(raw, z, offs, B, STEP, bg)[0]
    target = torch.cat([rgb, torch.ones(B, 1, device=DEV)], 1)
    loss, d_raw, rgb2 = render.composite_packed_mse_backward_bg(raw, offs, B, STEP, target, bg, need_rgb=True)
    assert float(loss) == 0.0 and float(d_raw.abs().max()) == 0.0 and bits_equal(rgb2, rgb)
    loss, dist, d_raw, _ = render.composite_packed_mse_dist_backward_bg(raw, z, offs, rays, STEP, S, target, bg, 1e-2)
    assert float(loss) == 0.0 and float(dist) > 0.0 and float(d_raw[:, :3].abs().max()) == 0.0 and float(d_raw[:, 3].abs().max()) > 0.0


@pytest.mark.parametrize("density", ["thin", "mixed", "saturated"])
def test_a_black_background_equals_no_background(density):
    """torch.equal: the values are equal, a zero may have changed its sign."""
    from nerf_meets_mlx_amd.rendering import render
    raw, z, offs, rays = _dev(*_batch(8, SIGMAS_BWD, density))
    rgba = _colours(9)[0].to(DEV)
    zeros = torch.zeros(B, 3, device=DEV)
    want = render.composite_packed(raw, z, offs, B, STEP, False)
    want_d = render.composite_packed_distortion(raw, z, offs, rays, STEP, S, False)
    assert bool(torch.isfinite(want[1]).all())
    for colour in (zeros, (0.0, 0.0, 0.0)):
        assert all(torch.equal(a, b) for a, b in zip(render.composite_packed_bg(raw, z, offs, B, STEP, colour), want))
        assert all(torch.equal(a, b) for a, b in zip(render.composite_packed_distortion_bg(raw, z, offs, rays, STEP, S, colour), want_d))
    t = rgba[:, :3] * rgba[:, 3:]                                # premultiplied colour
    _, d_raw, rgb = render.composite_packed_mse_backward_bg(raw, offs, B, STEP, rgba, zeros, need_rgb=True)
    _, w_d, w_rgb = render.composite_packed_mse_backward(raw, offs, B, STEP, t, False, need_rgb=True)
    assert torch.equal(d_raw, w_d) and torch.equal(rgb, w_rgb)
    _, _, d_raw, rgb = render.composite_packed_mse_dist_backward_bg(raw, z, offs, rays, STEP, S, rgba, zeros, 0.3, need_rgb=True)
    _, _, w_d, w_rgb = render.composite_packed_mse_dist_backward(raw, z, offs, rays, STEP, S, t, 0.3, False, need_rgb=True)
    assert torch.equal(d_raw, w_d) and torch.equal(rgb, w_rgb)


# ------------------------------------------------------------------------------------------------ 3: poisoned buffers
def test_every_output_is_written_and_nothing_outside():
    from nerf_meets_mlx_amd import _native as N
    raw, z, offs, rays = _dev(*_batch(10, SIGMAS_BWD, "mixed"))
    rgba, bg = (t.to(DEV) for t in _colours(11))
    K, PAD = raw.shape[0], 8
    lib = N.lib()

    def guarded(rows, cols):
        full = sentinel_(torch.empty(rows + 2 * PAD, cols, dtype=torch.float32, device=DEV))
        return full, full[PAD:PAD + rows]

    def check(full, inner, what):
        assert unwritten(inner) == 0, what
        assert unwritten(full) == 2 * PAD * full.shape[1], what

    ref = {}
    for dist_on in (False, True):
        bufs = {k: guarded(B, c) for k, c in (("rgb", 3), ("acc", 1), ("depth", 1), ("dist", 1))}
        o = [N.ptr(bufs[k][1]) for k in ("rgb", "acc", "depth", "dist")]
        if dist_on:
            N.check(lib.nerf_composite_packed_distortion_bg(N.ptr(raw), N.ptr(z), N.ptr(offs), N.ptr(rays), B, K, STEP, S, N.ptr(bg), 3,
                                                            *o, N.stream()))
        else:
            N.check(lib.nerf_composite_packed_forward_bg(N.ptr(raw), N.ptr(z), N.ptr(offs), B, K, STEP, N.ptr(bg), 3, *o[:3], N.stream()))
        for k, (full, inner) in bufs.items():
            if k != "dist" or dist_on:
                check(full, inner, f"forward dist={dist_on} {k}")
        ref[dist_on] = bufs
        # NULL acc / depth
        _, rgb_only = guarded(B, 3)
        _, dist_only = guarded(B, 1)
        if dist_on:
            N.check(lib.nerf_composite_packed_distortion_bg(N.ptr(raw), N.ptr(z), N.ptr(offs), N.ptr(rays), B, K, STEP, S, N.ptr(bg), 3,
                                                            N.ptr(rgb_only), None, None, N.ptr(dist_only), N.stream()))
            assert bits_equal(dist_only, bufs["dist"][1])
        else:
            N.check(lib.nerf_composite_packed_forward_bg(N.ptr(raw), N.ptr(z), N.ptr(offs), B, K, STEP, N.ptr(bg), 3, N.ptr(rgb_only),
                                                         None, None, N.stream()))
        assert bits_equal(rgb_only, bufs["rgb"][1])

    def train(dist_on, loss, dist, rgb, d_raw, raw_=raw, z_=z, offs_=offs, K_=K):
        if dist_on:
            N.check(lib.nerf_composite_packed_mse_dist_backward_bg(N.ptr(raw_), N.ptr(z_), N.ptr(offs_), N.ptr(rays), B, K_, STEP, S,
                                                                   N.ptr(rgba), N.ptr(bg), 1.0, 1e-2, N.ptr(loss), N.ptr(dist), N.ptr(rgb),
                                                                   N.ptr(d_raw), N.stream()))
        else:
            N.check(lib.nerf_composite_packed_mse_backward_bg(N.ptr(raw_), N.ptr(offs_), B, K_, STEP, N.ptr(rgba), N.ptr(bg), 1.0,
                                                              N.ptr(loss), N.ptr(rgb), N.ptr(d_raw), N.stream()))

    for dist_on in (False, True):
        d_full, d_in = guarded(K, 4)
        r_full, r_in = guarded(B, 3)
        loss, dist = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        train(dist_on, loss, dist, r_in, d_in)
        check(d_full, d_in, f"training dist={dist_on} d_raw")
        check(r_full, r_in, f"training dist={dist_on} rgb")
        assert float(loss) > 0.0 and (float(dist) > 0.0) == dist_on
        assert bits_equal(r_in, ref[dist_on]["rgb"][1])          # the training forms render the forward's rgb
        d2_full, d2_in = guarded(K, 4)                           # NULL loss, dist_out, rgb
        train(dist_on, None, None, None, d2_in)
        check(d2_full, d2_in, "training, NULL optional outputs")
        assert bits_equal(d2_in, d_in)
        # rays without any sample (K = 0): loss is the error of the background against the target, nothing else is touched
        o0 = torch.zeros(B + 1, dtype=torch.int64, device=DEV)
        r0_full, r0_in = guarded(B, 3)
        loss.zero_()
        train(dist_on, loss, dist, r0_in, None, raw_=None, z_=None, offs_=o0, K_=0)
        check(r0_full, r0_in, "training K = 0 rgb")
        assert bits_equal(r0_in, bg)
        a = rgba[:, 3:]
        want = float(((bg - (rgba[:, :3] * a + bg * (1.0 - a))).double() ** 2).mean())
        assert abs(float(loss) - want) <= 1e-5 * want
    # no rays
    assert lib.nerf_composite_packed_forward_bg(None, None, None, 0, 0, STEP, None, 0, None, None, None, N.stream()) == 0
    assert lib.nerf_composite_packed_mse_backward_bg(None, None, 0, 0, STEP, None, None, 1.0, None, None, None, N.stream()) == 0


# ------------------------------------------------------------------------------------------------ 4: edge cases
def test_nan_inf_and_bad_offsets_stay_in_their_own_ray():
    from nerf_meets_mlx_amd.rendering import render
    raw, z, offs, rays = _batch(12, SIGMAS_BWD, "mixed")
    rgba, bg = _colours(13)
    K = raw.shape[0]
    lam = 0.25

    def run(raw_, offs_, rgba_, bg_):
        a = _dev(raw_, z, offs_, rays)
        out = list(render.composite_packed_bg(a[0], a[1], a[2], B, STEP, bg_.to(DEV)))                               # rgb, acc, depth
        out.append(render.composite_packed_distortion_bg(*a, STEP, S, bg_.to(DEV))[3])                                # dist
        out.append(render.composite_packed_mse_backward_bg(a[0], a[2], B, STEP, rgba_.to(DEV), bg_.to(DEV))[1])       # d_raw
        out.append(render.composite_packed_mse_dist_backward_bg(*a, STEP, S, rgba_.to(DEV), bg_.to(DEV), lam)[2])     # d_raw + dist
        return out

    base = run(raw, offs, rgba, bg)
    assert all(bool(torch.isfinite(t).all()) for t in base)      # sigma = +inf samples included
    assert int((raw[:, 3] == 1e30).sum()) > 0
    seg = lambda b: slice(int(offs[b]), int(offs[b + 1]))        # noqa: E731

    def others(bs):
        keep_r, keep_k = torch.ones(B, dtype=torch.bool), torch.ones(K, dtype=torch.bool)
        for b in bs:
            keep_r[b] = False
            keep_k[seg(b)] = False
        return keep_r.to(DEV), keep_k.to(DEV)

    def same_elsewhere(got, bs, what):
        kr, kk = others(bs)
        for i, (g, w) in enumerate(zip(got, base)):
            k = kk if g.shape[0] == K else kr
            assert bits_equal(g[k], w[k]), (what, i)

    for what, b in (("bg", 7), ("bg", 0), ("target", 8), ("alpha", 3), ("raw", 5)):
        raw_n, rgba_n, bg_n = raw.clone(), rgba.clone(), bg.clone()
        if what == "bg":
            bg_n[b, 1] = float("nan")
        elif what == "target":
            rgba_n[b, 0] = float("nan")
        elif what == "alpha":
            rgba_n[b, 3] = float("nan")
        else:
            raw_n[int(offs[b]) + 3, 3] = float("nan")
        got = run(raw_n, offs, rgba_n, bg_n)
        same_elsewhere(got, [b], (what, b))
        if LENGTHS[b]:
            assert bool(torch.isnan(got[4][seg(b)]).any()) and bool(torch.isnan(got[5][seg(b)]).any()), (what, b)
        if what in ("bg", "raw"):
            assert bool(torch.isnan(got[0][b]).any()), (what, b)
        else:                                                    # the target does not enter the forward
            assert bits_equal(got[0], base[0])
    # bad offsets: rays 4 (ends beyond K) and 5 (decreasing) get NaN outputs, nobody else changes
    offs_b = offs.clone()
    offs_b[5] = K + 10
    got = run(raw, offs_b, rgba, bg)
    same_elsewhere(got, [4, 5], "offsets")
    assert all(bool(torch.isnan(got[i][[4, 5]]).all()) for i in range(4))
    # an infinite background colour poisons its own ray only (inf * 0 where acc = 1, inf elsewhere)
    bg_i = bg.clone()
    bg_i[8] = float("inf")
    same_elsewhere(run(raw, offs, rgba, bg_i), [8], "inf bg")


# ------------------------------------------------------------------------------------------------ 5: reproducibility
def test_bit_reproducible_over_launches_and_under_a_permutation_of_the_rays():
    from nerf_meets_mlx_amd.rendering import render
    raw, z, offs, rays = _batch(14, SIGMAS_BWD, "mixed")
    rgba, bg = _colours(15)

    def run(raw_, z_, offs_, rays_, rgba_, bg_):
        a = _dev(raw_, z_, offs_, rays_)
        c = (rgba_.to(DEV), bg_.to(DEV))
        rgb = render.composite_packed_bg(a[0], a[1], a[2], B, STEP, c[1])[0]
        d1 = render.composite_packed_mse_backward_bg(a[0], a[2], B, STEP, *c)[1]
        d2 = render.composite_packed_mse_dist_backward_bg(*a, STEP, S, *c, 0.1)[2]
        return rgb, d1, d2

    rgb, d1, d2 = run(raw, z, offs, rays, rgba, bg)
    for _ in range(3):
        assert all(bits_equal(a, b) for a, b in zip(run(raw, z, offs, rays, rgba, bg), (rgb, d1, d2)))
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(16))
    segs = [slice(int(offs[b]), int(offs[b + 1])) for b in perm.tolist()]
    raw_p, z_p = torch.cat([raw[s] for s in segs]), torch.cat([z[s] for s in segs])
    offs_p = torch.zeros(B + 1, dtype=torch.int64)
    offs_p[1:] = torch.cumsum(torch.tensor([LENGTHS[b] for b in perm.tolist()]), 0)
    rgb_p, d1_p, d2_p = run(raw_p, z_p, offs_p, rays[perm], rgba[perm], bg[perm])
    assert bits_equal(rgb_p, rgb[perm.to(DEV)])
    assert bits_equal(d1_p, torch.cat([d1[s] for s in segs])) and bits_equal(d2_p, torch.cat([d2[s] for s in segs]))


# ------------------------------------------------------------------------------------------------ 6: early termination
def test_early_termination_over_a_background():
    from nerf_meets_mlx_amd import _native as N
    from nerf_meets_mlx_amd.rendering import render
    f = _field()
    g = _grid(f, 256)
    _random_bits(g, 0.6, 10)
    dense = _Dense(f, 2.0)
    n = 3000
    rays = _rays(n, 8)
    gen = torch.Generator().manual_seed(17)
    jit, bg = torch.rand(n, generator=gen).float().to(DEV), torch.rand(n, 3, generator=gen).float().to(DEV)
    keys = ("rgb", "acc", "depth", "samples")

    def run(r, j, c, eps=1e-2, **kw):
        o = g.render_ert(dense, r, j, eps, True, background=c, **kw)         # white_bkgd is overridden by the background
        return [o[k].clone() for k in keys]

    ref = run(rays, jit, bg)
    assert g.last_ert["rounds"] > 1
    # the result does not depend on round sizes, chunking or ray order
    chunks = [run(rays[s:s + 1000], jit[s:s + 1000], bg[s:s + 1000]) for s in range(0, n, 1000)]
    rev = [t.flip(0) for t in run(rays.flip(0).contiguous(), jit.flip(0).contiguous(), bg.flip(0).contiguous())]
    for v in ([torch.cat([c[i] for c in chunks]) for i in range(4)], rev, run(rays, jit, bg, slots=1), run(rays, jit, bg, slots=64)):
        for a, b in zip(v, ref):
            assert bits_equal(a.view(torch.int32), b.view(torch.int32))
    # the finish is the state's colour plus (1 - acc) * bg in float32, and one colour for all rays is the per-ray form's bits
    plain = g.render_ert(dense, rays, jit, 1e-2, False)
    ok = torch.isfinite(plain["acc"])
    assert int(ok.sum()) > n // 2
    assert bits_equal(ref[0][ok], (plain["rgb"] + (1.0 - plain["acc"])[:, None] * bg)[ok]) and bits_equal(ref[1], plain["acc"])
    one = run(rays, jit, (0.25, 0.5, 0.75))
    per = run(rays, jit, torch.tensor([0.25, 0.5, 0.75], device=DEV).expand(n, 3).contiguous())
    assert all(bits_equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(one, per))
    white = g.render_ert(dense, rays, jit, 1e-2, True)
    assert bits_equal(run(rays, jit, (1.0, 1.0, 1.0))[0], white["rgb"])
    # at eps = 0 it is the one-shot render over the same background (the field of test_gpu_ert's eps = 0 test)
    ro = g.render_ert(f, rays, jit, 0.0, True, background=bg)
    o = [ro[k].clone() for k in keys]
    offs, rows, z, K = g.march(rays, jit)
    w_rgb, w_acc, _ = render.composite_packed_bg(f.query_packed(rows, z), z, offs, n, g.step_world, bg)
    assert K > 0 and bool(torch.isfinite(w_rgb).all())
    assert float((o[0] - w_rgb).abs().max()) <= 2e-6 and float((o[1] - w_acc).abs().max()) <= 2e-6
    assert torch.equal(o[3].long(), offs[1:] - offs[:-1])
    # every output of the finish is written; NULL optional outputs
    ist, fst = g._cull["ert_istate"][:4 * n].view(n, 4), g._cull["ert_fstate"][:6 * n].view(n, 6)
    outs = [sentinel_(torch.empty(*s, dtype=torch.float32, device=DEV)) for s in ((n, 3), (n,), (n,), (n,))]
    N.check(N.lib().nerf_ert_finish_bg(N.ptr(ist), N.ptr(fst), n, N.ptr(bg), 3, *(N.ptr(t) for t in outs), N.stream()))
    assert all(unwritten(t) == 0 for t in outs) and bits_equal(outs[0], o[0])
    rgb_only = sentinel_(torch.empty(n, 3, dtype=torch.float32, device=DEV))
    N.check(N.lib().nerf_ert_finish_bg(N.ptr(ist), N.ptr(fst), n, N.ptr(bg), 3, N.ptr(rgb_only), None, None, None, N.stream()))
    assert bits_equal(rgb_only, o[0])


# ------------------------------------------------------------------------------------------------ 7: the RGBA sampler
def test_rgba_sampler_draws_the_pixels_and_rays_of_the_rgb_sampler():
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.rendering import ray
    H, W = 37, 53
    K, _ = synthetic.intrinsics(H, W)
    c2w = synthetic.train_poses(1, 3)[0][:3, :4]
    img = torch.rand(H, W, 4, generator=torch.Generator().manual_seed(18)).to(DEV)
    rgb = img[..., :3].contiguous()
    for n, seed, offset in ((256, 5, 0), (H * W, 6, 0), (100, 2 ** 63 + 11, 1000), (1, 7, H * W - 1)):
        r3, t3, i3 = ray.sample_batch(H, W, K, c2w, 2.0, 6.0, rgb, n, seed, offset, return_idx=True)
        r4, t4, i4 = ray.sample_batch(H, W, K, c2w, 2.0, 6.0, img, n, seed, offset, return_idx=True)
        assert bits_equal(r4, r3) and torch.equal(i4, i3) and tuple(t4.shape) == (n, 4)
        assert bits_equal(t4, img.reshape(-1, 4)[i4]) and bits_equal(t4[:, :3].contiguous(), t3)
    # every output written and nothing outside it
    from nerf_meets_mlx_amd import _native as N
    n, PAD = 300, 8
    bufs = [sentinel_(torch.empty(n + 2 * PAD, c, dtype=torch.float32, device=DEV)) for c in (11, 4)]
    idx = torch.full((n + 2 * PAD,), -7, dtype=torch.int64, device=DEV)
    Kc, cc = ray._host_cam(K, c2w)
    N.check(N.lib().nerf_sample_batch_rgba(n, H, W, 5, 0, Kc, cc, 2.0, 6.0, N.ptr(img), N.ptr(bufs[0][PAD:PAD + n]),
                                           N.ptr(bufs[1][PAD:PAD + n]), N.ptr(idx[PAD:PAD + n]), N.stream()))
    for t in bufs:
        assert unwritten(t[PAD:PAD + n]) == 0 and unwritten(t) == 2 * PAD * t.shape[1]
    assert int((idx == -7).sum()) == 2 * PAD and int(torch.unique(idx[PAD:PAD + n]).numel()) == n
    r4, t4 = ray.sample_batch(H, W, K, c2w, 2.0, 6.0, img, 64, 9)           # pixel_idx NULL
    r3, _ = ray.sample_batch(H, W, K, c2w, 2.0, 6.0, rgb, 64, 9)
    assert bits_equal(r4, r3)
    with pytest.raises(ValueError):
        ray.sample_batch(H, W, K, c2w, 2.0, 6.0, img[..., :2].contiguous(), 64, 9)


# ------------------------------------------------------------------------------------------------ 8: trainers
def _trainer(imgs, poses, K, rbg, weight=None):
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    return NGPTrainer(imgs[:-1], poses[:-1], K, N_rand=256, n_depth_samples=64, seed=4, device=DEV, log2_hashmap_size=14,
                      occupancy_grid=True, march_steps=1024, random_background=rbg, distortion_weight=weight)


def _state(tr):
    f = tr.field
    return [f.mlp.params.clone(), f.enc.tables.clone()] + [t.clone() for k in ("mlp", "tables") for t in tr.opt.state[k]] + \
        [tr.grid.density.clone(), tr.grid.bits.clone()]


def test_trainer_batches_and_explicit_backgrounds():
    """sample_batch of an RGBA trainer gives the 3-channel trainer's pixels and rays; train_step draws bg from counter stream 5;
    an explicit (rays, target, background) step is that step; the keyword composes with distortion_weight."""
    from nerf_meets_mlx_amd import parallel
    from nerf_meets_mlx_amd.dataset import synthetic
    imgs3, poses, _, _, K = synthetic.make_dataset(48, 48, 9, seed=0, device=DEV)
    imgs4 = synthetic.make_dataset(48, 48, 9, seed=0, device=DEV, rgba=True)[0]
    w, a, b = _trainer(imgs3, poses, K, False), _trainer(imgs4, poses, K, True), _trainer(imgs4, poses, K, True)
    d = _trainer(imgs4, poses, K, True, 1e-2)
    for it in range(3):
        r3, t3 = w.sample_batch()
        r4, t4 = a.sample_batch()
        assert bits_equal(r3, r4) and tuple(t4.shape) == (256, 4)
        al = t4[:, 3:]
        assert float((t4[:, :3] * al + (1.0 - al) - t3).abs().max()) <= 1e-6
        idx = torch.arange(0, 2000, 9, device=DEV)
        assert bits_equal(a.sample_batch(pixel_idx=idx, img_i=2)[1], imgs4[2].reshape(-1, 4)[idx])
        gen = torch.Generator(device=DEV)
        gen.manual_seed(parallel.counter_seed(4, 0, 5, it))
        bg = torch.rand(256, 3, dtype=torch.float32, device=DEV, generator=gen)
        assert float(bg.min()) >= 0.0 and float(bg.max()) < 1.0
        oa = a.train_step()
        ob = b.train_step(r4, t4, background=bg)
        assert set(oa) == set(ob) == {"loss_coarse"}
        for x, y in zip(_state(a), _state(b)):
            assert bits_equal(x, y)
        w.train_step()
        assert set(d.train_step()) == {"loss_coarse", "loss_distortion"}
    with pytest.raises(ValueError, match="random_background"):
        w.train_step(r3, t3, background=bg)


def test_trainers_over_white_and_over_random_backgrounds():
    """The set-up of the existing trainer tests (hw 48, 9 views with the last held out, 2^14-entry tables, seed 4, 256 rays per
    step, march_steps 1024, 600 iterations): a white arm (3-channel images, the code path before this feature) beside a
    random-background arm on the same scene as RGBA.  (a) the white arm's first 32 steps are bit-identical to a second white
    trainer's; (b) two random-background runs are bit-identical, the grid included; (c) a checkpoint written at iteration 300 and
    loaded into a fresh trainer gives a bit-identical state at iteration 332; (d) the random-background arm has not collapsed: over
    white, its held-out PSNR beats the all-white frame by at least half of the white arm's margin; (e) over a black background,
    against the teacher's RGBA frame, the random-background arm scores strictly higher than the white arm.  The figures measured
    on an MI355X are in DESIGN.md section 16."""
    import os
    import tempfile
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.rendering import ray
    imgs3, poses, _, _, K = synthetic.make_dataset(48, 48, 9, seed=0, device=DEV)
    imgs4 = synthetic.make_dataset(48, 48, 9, seed=0, device=DEV, rgba=True)[0]
    gt_white, gt_rgba, pose = imgs3[-1], imgs4[-1], poses[-1]
    gt_black = gt_rgba[..., :3] * gt_rgba[..., 3:]               # the teacher's frame over black: premultiplied colour
    white, white2 = _trainer(imgs3, poses, K, False), _trainer(imgs3, poses, K, False)
    ra, rb, rc = _trainer(imgs4, poses, K, True), _trainer(imgs4, poses, K, True), _trainer(imgs4, poses, K, True)
    logged, at332 = [], None
    with tempfile.TemporaryDirectory() as tmp:
        for it in range(600):
            o = white.train_step()
            orb = ra.train_step()
            rb.train_step()
            assert set(o) == set(orb) == {"loss_coarse"}
            if it < 32:
                white2.train_step()
            if it == 31:
                for x, y in zip(_state(white), _state(white2)):
                    assert bits_equal(x, y)                      # (a)
            if it == 299:
                path = ra.save(os.path.join(tmp, "rbg"))
                assert rc.load(path) == 300
            if 300 <= it < 332:
                rc.train_step()
            if it == 331:
                at332 = _state(ra)
                for x, y in zip(at332, _state(rc)):
                    assert bits_equal(x, y)                      # (c)
            if it % 100 == 99:
                logged.append((it + 1, float(o["loss_coarse"]), float(orb["loss_coarse"])))
    assert at332 is not None and all(np.isfinite(v) for row in logged for v in row)
    for x, y in zip(_state(ra), _state(rb)):
        assert bits_equal(x, y)                                  # (b)
    c2w = pose[:3, :4].numpy()
    rays = ray.gen_rays(48, 48, white.K, c2w, 2.0, 6.0, torch.arange(48 * 48, device=DEV, dtype=torch.int64))
    black = (0.0, 0.0, 0.0)
    p_white = {n: t.psnr(c2w, gt_white) for n, t in (("white", white), ("rbg", ra))}
    p_black = {n: t.psnr(c2w, gt_black, background=black) for n, t in (("white", white), ("rbg", ra))}
    p_all_white = float(-10.0 * torch.log10(((1.0 - gt_white.double()) ** 2).mean()))
    a_gt = gt_rgba[..., 3].reshape(-1)
    fig = {}
    for n, t in (("white", white), ("rbg", ra)):
        aux = t.render_rays(rays, aux=True)
        assert set(aux) == {"rgb", "acc", "depth", "samples"}
        assert bits_equal(aux["rgb"], t.render_rays(rays, background=(1.0, 1.0, 1.0)))       # white_bkgd is the colour (1, 1, 1)
        rgba = t.render_rays(rays, aux=True, background=black)                               # an RGBA frame
        assert bits_equal(rgba["acc"], aux["acc"]) and bits_equal(rgba["rgb"], t.render_frame(c2w, background=black).reshape(-1, 3))
        per_ray = t.render_rays(rays, background=torch.zeros(48 * 48, 3, device=DEV))
        assert bits_equal(per_ray, rgba["rgb"])
        t.min_transmittance = 1e-4
        try:
            ert = t.render_rays(rays, aux=True, background=black)
        finally:
            t.min_transmittance = None
        d_acc = rgba["acc"] - ert["acc"]                         # the header's bound: 0 <= acc_full - acc_eps < eps, up to rounding
        assert float(d_acc.min()) >= -4e-6 and float(d_acc.max()) < 1e-4 + 4e-6
        fig[n] = {"alpha_mae": float((aux["acc"] - a_gt).abs().double().mean()), "acc": float(aux["acc"].double().mean()),
                  "white_share": float((aux["rgb"] > 0.999).all(-1).double().mean()),
                  "samples": float(aux["samples"].double().mean()), "samples_ert": float(ert["samples"].double().mean())}
    print(f"\nbackground trainers hw48, 600 it: held-out PSNR over white: white arm {p_white['white']:.2f} random-bg arm "
          f"{p_white['rbg']:.2f} all-white frame {p_all_white:.2f}; over black: white arm {p_black['white']:.2f} random-bg arm "
          f"{p_black['rbg']:.2f}; teacher mean alpha {float(a_gt.double().mean()):.3f}, white-pixel share "
          f"{float((gt_white.reshape(-1, 3) > 0.999).all(-1).double().mean()):.3f}; (alpha MAE, mean acc, white-pixel share, samples/ray, "
          f"samples/ray at eps 1e-4) white arm {fig['white']} random-bg arm {fig['rbg']}; (it, mse white, mse random-bg) {logged}")
    assert p_white["white"] > p_all_white, (p_white, p_all_white)
    assert p_white["rbg"] - p_all_white >= 0.5 * (p_white["white"] - p_all_white), (p_white, p_all_white)      # (d)
    assert p_black["rbg"] > p_black["white"], p_black                                                            # (e)
