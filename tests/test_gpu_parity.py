"""GPU parity tests: the HIP path (package wrappers -> C ABI -> gfx950 kernels) against the
CPU oracle on identical seeded inputs, and against the reference-run golden fixtures.

Tolerances (stated per test):
  * integer / index outputs: bit-exact.
  * float32 kernels (rays, sampling, compositing, encoders, Adam): a few ulp, written as atol/rtol IN THIS FILE.  The same units are
    held bit for bit to float32 host mirrors elsewhere: ray generation, the fused batch, the NDC warp and the row gather in
    tests/test_gpu_rays.py; depth sampling, the importance sampler and the MSE gradient in tests/test_gpu_render.py (compositing
    within a derived expf bound); the hash grid in tests/test_gpu_hashgrid.py; SSIM on its float64 sums within a derived
    summation bound in tests/test_gpu_ssim.py.
  * the MLP at the DEFAULT precision (22: the reference's float32 tolerance, split 16-bit MFMA operands) vs the pure float32
    oracle: rel-to-max 1e-4 on network outputs, 1e-3-class bars on rendered / trained quantities (stated per test).
  * the MLP at precision=16 (bf16 MFMA operands: the DECLARED reduced-precision mode, opt-in; the `mlp_variant` kernels of
    round 1 are all of this kind): vs the oracle with bf16 operand rounding emulated (same rounding points, fp32 accumulate)
    rel-to-max 1e-2; vs the pure fp32 oracle rel-to-max 3e-2 -- bf16 has 8 bits of mantissa and the error random-walks over
    12 layers.  Tests of that mode say `precision=16` explicitly.
"""
import os

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from nerf_meets_mlx_amd import _native
    assert _native.lib().nerf_abi_version() == 3        # fails loudly if the .so is missing


def _relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _lego_K(H, W):
    f = 0.5 * W / np.tan(0.5 * 0.6911112070083618)
    return np.array([[f, 0, 0.5 * W], [0, f, 0.5 * H], [0, 0, 1]], dtype=np.float64)


# ------------------------------------------------------------------------------ a3 / K12
def test_pixel_permutation_bit_exact():
    from nerf_meets_mlx_amd.ops import index
    for n, dom, seed, off in [(1024, 640000, 7, 0), (4096, 160000, 123456789, 1000), (1000, 1000, 3, 0), (5, 7, 1, 2)]:
        dev = index.pixel_permutation(n, dom, seed, off, DEV).cpu().numpy()
        host = index.pixel_permutation_host(n, dom, seed, off)
        assert np.array_equal(dev, host)
        assert len(set(dev.tolist())) == n and dev.min() >= 0 and dev.max() < dom
    with pytest.raises(ValueError):
        index.pixel_permutation(10, 5, 0, 0, DEV)


# ------------------------------------------------------------------------------ a1 / a4
def test_ray_gen_matches_oracle_and_reference(golden_dir):
    from nerf_meets_mlx_amd.rendering import ray
    g = np.load(os.path.join(golden_dir, "ref_get_rays.npz"))
    H, W = (int(v) for v in g["lego800_HW"])
    idx = torch.from_numpy(g["lego800_idx"]).to(DEV)
    rays, coords = ray.gen_rays(H, W, g["lego800_K"], g["lego800_c2w"], 2.0, 6.0, idx, return_coords=True)
    rays = rays.cpu()
    # reference get_rays evaluates in float64 (float64 K); ours rounds that once to float32
    assert torch.equal(rays[:, 3:6], torch.from_numpy(g["lego800_d"]).float())
    assert torch.equal(rays[:, 0:3], torch.from_numpy(g["lego800_o"]).float())
    assert torch.equal(coords.cpu(), O.select_coords(idx.cpu(), W))                   # integer, bit-exact
    want = O.pack_rays(rays[:, 0:3], rays[:, 3:6], 2.0, 6.0)
    np.testing.assert_allclose(rays.numpy(), want.numpy(), rtol=0, atol=2e-7)
    # whole small image through the reference-shaped API
    for case in ("small", "rect", "lego64"):
        h, w = (int(v) for v in g[f"{case}_HW"])
        o, d = ray.get_rays(h, w, g[f"{case}_K"], g[f"{case}_c2w"])
        assert o.shape == (h, w, 3)
        assert torch.equal(d.cpu(), torch.from_numpy(g[f"{case}_d"]).float())
    # empty index list
    assert ray.gen_rays(H, W, g["lego800_K"], g["lego800_c2w"], 2.0, 6.0, idx[:0]).shape == (0, 11)


def test_ndc_rays():
    from nerf_meets_mlx_amd.rendering import ray
    torch.manual_seed(0)
    o = torch.randn(100, 3); o[:, 2] -= 4.0
    d = torch.randn(100, 3); d[:, 2] = -d[:, 2].abs() - 0.5
    wo, wd = O.ndc_rays(378, 504, 400.0, 1.0, o, d)
    go, gd = ray.ndc_rays(378, 504, 400.0, 1.0, o.to(DEV), d.to(DEV))
    np.testing.assert_allclose(go.cpu().numpy(), wo.numpy(), rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(gd.cpu().numpy(), wd.numpy(), rtol=2e-5, atol=2e-6)


# ------------------------------------------------------------------------------ a5-a7
def test_sample_coarse():
    from nerf_meets_mlx_amd import sampling
    from nerf_meets_mlx_amd.sampling import uniform, linear_disparity
    B, n = 37, 64
    near = torch.full((B, 1), 2.0); far = torch.full((B, 1), 6.0)
    far[3] = 7.5; near[5] = 0.5
    z = uniform.sample_z(near.to(DEV), far.to(DEV), n).cpu()
    assert torch.equal(z, O.sample_z_uniform(near, far, n))                            # same fp32 op sequence
    zl = linear_disparity.sample_z(near.to(DEV), far.to(DEV), 16).cpu()
    wl = O.sample_z_lindisp(near, far, 16)
    np.testing.assert_allclose(zl.numpy(), wl.numpy(), rtol=1e-6, atol=0)
    assert float(zl[0, 0]) == 0.0 and float(zl[0, -1]) == 0.0                           # Q12 literal
    t = torch.rand(B, n)
    rays = torch.zeros(B, 11); rays[:, 6:7] = near; rays[:, 7:8] = far
    zj = sampling.sample_coarse(rays.to(DEV), n, perturb=1.0, t_rand=t.to(DEV)).cpu()
    np.testing.assert_allclose(zj.numpy(), O.add_noise_z(O.sample_z_uniform(near, far, n), 1.0, t).numpy(), rtol=0, atol=5e-7)
    assert torch.equal(sampling.add_noise_z(z, 0.0), z)
    # the stand-alone form on caller-supplied (here: unevenly spaced) depths runs the same arithmetic as a kernel
    zz = torch.sort(torch.rand(37, 19) * 4 + 2, -1).values
    tt = torch.rand(37, 19)
    for strength in (1.0, 0.3):
        got = sampling.add_noise_z(zz.to(DEV), strength, tt.to(DEV)).cpu()
        np.testing.assert_allclose(got.numpy(), O.add_noise_z(zz, strength, tt).numpy(), rtol=0, atol=5e-7)
    one = sampling.add_noise_z(zz[:, :1].contiguous().to(DEV), 1.0, tt[:, :1].contiguous().to(DEV)).cpu()
    assert torch.equal(one, zz[:, :1])                      # n = 1: lower == upper == z


# ------------------------------------------------------------------------------ a15 / a17
@pytest.mark.parametrize("tag", ["const", "zero", "peaky", "spike", "jitter", "small", "signed"])
def test_importance_sampler_vs_reference_fixture(golden_dir, tag):
    from nerf_meets_mlx_amd import sampling
    g = np.load(os.path.join(golden_dir, "ref_inverse_cdf.npz"))
    z, w, u, ref = (torch.from_numpy(g[f"{tag}_{k}"]) for k in ("z", "w", "u", "out"))
    Nn = u.shape[-1]
    z_new, z_m, cdf, inds = sampling.importance_sample(z.to(DEV), w.to(DEV), Nn, u=u.to(DEV), return_parts=True)
    z_new, z_m, cdf, inds = z_new.cpu(), z_m.cpu(), cdf.cpu(), inds.cpu()
    _, o_cdf, o_inds, _, _ = O.inverse_cdf_parts(z, w, u)
    if tag != "signed":   # negative weights cannot come out of raw2outputs (alpha >= 0, T > 0); the fixture's
        # near-zero weight sum makes the cdf cancel catastrophically -> only consistency is checked there
        np.testing.assert_allclose(cdf.numpy(), o_cdf.numpy(), rtol=0, atol=2.5e-7)      # sum order differs by <= 2 ulp
    # integer outputs: bit-exact given (cdf, u)
    assert torch.equal(inds, torch.searchsorted(cdf, u.contiguous(), side="right"))
    same = inds == o_inds
    assert torch.isfinite(z_new).all()
    if tag != "signed":
        assert same.float().mean() > 0.995                                               # u within 1 ulp of a cdf knot
        np.testing.assert_allclose(z_new[same].numpy(), ref[same].numpy(), rtol=0, atol=2e-5)
        assert float((z_new - ref).abs().max()) < 1e-3
    # merge: exact multiset of the inputs, ascending
    want = torch.sort(torch.cat([z, z_new], -1), -1).values
    assert torch.equal(z_m, want)
    # reference-shaped entry point
    z2 = sampling.sample_from_inverse_cdf_torch(z.to(DEV), w.to(DEV), Nn, u=u.to(DEV)).cpu()
    assert torch.equal(z2, z_new)


def test_importance_sampler_shapes_and_errors():
    from nerf_meets_mlx_amd import sampling
    torch.manual_seed(1)
    for B, n, Nn in [(1, 2, 1), (5, 100, 37), (3, 192, 64), (2, 256, 512)]:
        z = torch.sort(torch.rand(B, n) * 4 + 2, -1).values
        w = torch.rand(B, n, 1) ** 3
        u = torch.rand(B, Nn)
        z_new, z_m = sampling.importance_sample(z.to(DEV), w.to(DEV), Nn, u=u.to(DEV))
        want = O.sample_from_inverse_cdf(z, w, u)
        assert float((z_new.cpu() - want).abs().max()) < 2e-3
        assert torch.equal(z_m.cpu(), torch.sort(torch.cat([z, z_new.cpu()], -1), -1).values)
    with pytest.raises(ValueError):
        sampling.importance_sample(torch.rand(2, 300, device=DEV), torch.rand(2, 300, device=DEV), 8)


# ------------------------------------------------------------------------------ a9 / a10 / a22 / a23
def test_embedder_and_sinusoidal():
    from nerf_meets_mlx_amd.models import embedding
    from nerf_meets_mlx_amd.encoding import SinusoidalEncoding, IdentityEncoding
    torch.manual_seed(2)
    x = (torch.rand(1000, 3) - 0.5) * 12.0                               # |x| <= 6 -> arguments up to 486 rad
    for L, quirk in [(10, True), (4, True), (10, False)]:
        fn, ch = embedding.get_embedder(L, ref_quirks=quirk)
        e = fn(x.to(DEV)).cpu()
        want = O.embedder(x, L, quirk)
        assert ch == want.shape[1]
        np.testing.assert_allclose(e.numpy(), want.numpy(), rtol=0, atol=2e-6)
    assert torch.all(e[:, :3] == x)
    pos = torch.randn(4, 8, 3); d = torch.nn.functional.normalize(torch.randn(4, 3), dim=-1)
    fp, _ = embedding.get_embedder(10); fd, _ = embedding.get_embedder(4)
    emb = embedding.embed(pos.to(DEV), fp, d.to(DEV), fd).cpu()
    np.testing.assert_allclose(emb.numpy(), O.embed(pos, d).numpy(), rtol=0, atol=2e-6)
    # image-learning encoder: integer pixel coordinates 0..399, freq up to 256 (config 1)
    xi = torch.stack([torch.randint(0, 400, (2500,)), torch.randint(0, 400, (2500,))], -1).float()
    enc = SinusoidalEncoding(2, 10, 0.0, 8.0, False)
    assert enc.get_out_dim() == 40
    out = enc(xi.to(DEV)).cpu()
    np.testing.assert_allclose(enc.freq_bands(), O.sinusoidal_freqs(10, 0.0, 8.0).numpy(), rtol=0, atol=0)
    np.testing.assert_allclose(out.numpy(), O.sinusoidal_encoding(xi, 10, 0.0, 8.0, False).numpy(), rtol=0, atol=3e-6)
    enc2 = SinusoidalEncoding(2, 6, None, None, True)
    np.testing.assert_allclose(enc2(xi.to(DEV)).cpu().numpy(), O.sinusoidal_encoding(xi, 6, None, None, True).numpy(), atol=3e-6)
    assert IdentityEncoding(3)(x) is x and IdentityEncoding(3).get_out_dim() == 3


def test_spherical_harmonics():
    from nerf_meets_mlx_amd.encoding import SphericalHarmonicsEncoding
    torch.manual_seed(3)
    d = torch.nn.functional.normalize(torch.randn(513, 3), dim=-1)
    d[:3] = torch.eye(3)
    for deg in range(5):
        enc = SphericalHarmonicsEncoding(3, deg)
        out = enc(d.to(DEV)).cpu()
        assert out.shape == (513, (deg + 1) ** 2)
        np.testing.assert_allclose(out.numpy(), O.sh_encoding(d, deg).numpy(), rtol=2e-6, atol=2e-7)
    with pytest.raises(AssertionError):
        SphericalHarmonicsEncoding(3, 5)


def test_hashgrid_forward_backward():
    from nerf_meets_mlx_amd.encoding import MultiHashEncoding
    torch.manual_seed(4)
    enc = MultiHashEncoding(3, 16, 16, 2048, 2, 19, device=DEV)
    assert enc.scaled_res == O.hashgrid_resolutions(16, 16, 2048) and enc.get_out_dim() == 32
    enc.tables = torch.randn_like(enc.tables)
    x = torch.rand(2000, 3)
    x[0] = torch.tensor([0.25, 0.5, 0.75]); x[1] = 0.0; x[2] = 1.0                  # lattice points: floor == ceil
    out = enc(x.to(DEV)).cpu()
    tab = enc.tables.cpu()
    want = O.hashgrid_encoding(x, tab, enc.scaled_res)
    np.testing.assert_allclose(out.numpy(), want.numpy(), rtol=1e-5, atol=1e-6)
    # backward: adjoint of the interpolation vs autograd on the oracle (small table so autograd is cheap)
    enc2 = MultiHashEncoding(3, 4, 4, 32, 4, 10, device=DEV)
    enc2.tables = torch.randn_like(enc2.tables)
    t2 = enc2.tables.cpu().double().requires_grad_(True)
    g = torch.randn(2000, 16)
    O.hashgrid_encoding(x.double(), t2, enc2.scaled_res).backward(g.double())
    got = enc2.backward(x.to(DEV), g.to(DEV)).cpu()
    np.testing.assert_allclose(got.numpy(), t2.grad.float().numpy(), rtol=2e-4, atol=2e-4)
    # many points, 16 levels, heavy collisions in a 2^10 table: every contribution must arrive
    enc3 = MultiHashEncoding(3, 16, 4, 256, 2, 10, device=DEV)
    xs = torch.rand(300000, 3) * 3 - 1.5
    g3 = torch.ones(300000, 32)
    got3 = enc3.backward(xs.to(DEV), g3.to(DEV)).cpu().double()
    # with unit upstream gradients every level's table receives sum of interpolation weights = number of points
    np.testing.assert_allclose(got3.sum(dim=(1, 2)).numpy(), np.full(16, 2 * 300000.0), rtol=1e-4)


# ------------------------------------------------------------------------------ a13
def _composite_inputs(B, n, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    z = torch.sort(torch.rand(B, n, generator=g) * 4 + 2, -1).values
    raw = torch.randn(B, n, 4, generator=g)
    raw[..., 3] = raw[..., 3] * 3.0                      # signed densities: exercises the un-ReLU'd T (Q10)
    d = torch.randn(B, 3, generator=g)
    return raw.to(dtype), z.to(dtype), d.to(dtype)


@pytest.mark.parametrize("n", [1, 2, 64, 65, 192, 300, 1024])
@pytest.mark.parametrize("white", [False, True])
def test_composite_forward(n, white):
    from nerf_meets_mlx_amd.rendering import render
    B = 33
    raw, z, d = _composite_inputs(B, n, 100 + n)
    raw[..., 3] = raw[..., 3].clamp(-0.5, 50)            # keep exp(+S) finite in fp32 for the comparison
    got = render.raw2outputs(raw.to(DEV), z.to(DEV), d.to(DEV), 0, white)
    want = O.raw2outputs(raw.double(), z.double(), d.double(), 0.0, white)
    names = ["rgb", "disp", "acc", "weights", "depth"]
    for nm, a, b in zip(names, got, want):
        assert a.shape == b.shape, nm
        if nm == "disp":
            continue                                     # 1/max(1e-10, depth/acc): ill-conditioned by design
        # float32 scan / exp vs float64: error grows with sum |x|; 2e-4 of the output scale covers n = 1024
        scale = float(b.abs().max()) + 1e-6
        assert float((a.cpu().double() - b).abs().max()) < 2e-4 * scale, nm


def test_composite_edge_cases():
    from nerf_meets_mlx_amd.rendering import render
    B, n = 4, 64
    z = torch.linspace(2.0, 6.0, n).expand(B, n).contiguous()
    d = torch.tensor([[0.0, 0.0, -1.0]]).expand(B, 3).contiguous()
    raw = torch.zeros(B, n, 4); raw[..., :3] = torch.tensor([0.2, 0.5, 0.9])
    rgb, disp, acc, w, depth = render.raw2outputs(raw.to(DEV), z.to(DEV), d.to(DEV), 0, True)
    assert torch.all(w == 0) and torch.all(rgb == 1.0) and torch.isnan(disp).all()          # sigma == 0 (Q11)
    raw[..., 3] = 1.7
    rgb, disp, acc, w, depth = render.raw2outputs(raw.to(DEV), z.to(DEV), d.to(DEV), 0, False)
    np.testing.assert_allclose(acc.cpu().numpy(), 1.0, atol=1e-5)
    np.testing.assert_allclose(rgb.cpu().numpy()[0], [0.2, 0.5, 0.9], atol=1e-5)
    # noise path: explicit N(0,1) tensor
    noise = torch.randn(B, n)
    got = render.raw2outputs(raw.to(DEV), z.to(DEV), d.to(DEV), 0.5, False, noise=noise.to(DEV))
    want = O.raw2outputs(raw, z, d, 0.5, False, noise=noise)
    np.testing.assert_allclose(got[0].cpu().numpy(), want[0].numpy(), atol=1e-5)
    assert render.raw2outputs(raw[:0].to(DEV), z[:0].to(DEV), d[:0].to(DEV))[0].shape == (0, 3)


@pytest.mark.parametrize("n,white", [(64, True), (192, False), (7, True)])
def test_composite_backward(n, white):
    from nerf_meets_mlx_amd.rendering import render
    B = 19
    raw, z, d = _composite_inputs(B, n, 7 + n)
    raw[..., 3] = raw[..., 3].clamp(-0.3, 30)
    rays = torch.zeros(B, 11); rays[:, 3:6] = d
    g_rgb, g_acc, g_dep = torch.randn(B, 3), torch.randn(B), torch.randn(B)
    rd = raw.double().requires_grad_(True)
    rgb, disp, acc, w, depth = O.raw2outputs(rd, z.double(), d.double(), 0.0, white)
    ((rgb * g_rgb.double()).sum() + (acc[:, 0] * g_acc.double()).sum() + (depth[:, 0] * g_dep.double()).sum()).backward()
    got = render.composite_backward(raw.to(DEV), z.to(DEV), rays.to(DEV), g_rgb.to(DEV), white, g_acc.to(DEV),
                                    g_dep.to(DEV)).cpu()
    want = rd.grad
    inner = slice(0, n - 1)
    # last sample: delta = 1e10 |d| multiplies the density gradient -> compare relatively
    np.testing.assert_allclose(got[:, inner].numpy(), want[:, inner].float().numpy(), rtol=2e-3, atol=2e-4 * float(want[:, inner].abs().max()))
    lw, lg = want[:, -1, 3], got[:, -1, 3].double()
    assert float(((lg - lw).abs() / (lw.abs() + 1e-3 * lw.abs().max() + 1e-30)).max()) < 5e-3
    np.testing.assert_allclose(got[:, -1, :3].numpy(), want[:, -1, :3].float().numpy(), rtol=2e-3, atol=1e-5)


def test_mse_psnr():
    from nerf_meets_mlx_amd.ops import metric
    p, t = torch.rand(1024, 3), torch.rand(1024, 3)
    np.testing.assert_allclose(float(metric.MSE()(p.to(DEV), t.to(DEV))), float(O.mse(p, t)), rtol=1e-5)
    np.testing.assert_allclose(float(metric.PSNR()(p.to(DEV), t.to(DEV))), float(O.psnr(p, t)), rtol=1e-5)
    loss, dp = metric.mse_loss_grad(p.to(DEV), t.to(DEV))
    np.testing.assert_allclose(dp.cpu().numpy(), (2 * (p - t) / p.numel()).numpy(), rtol=1e-6, atol=1e-9)


# ------------------------------------------------------------------------------ a11 / a12
def _model_pair(seed=0, scale=1.0, precision=16):
    """precision=None: the constructor's default (22, held to the float32 oracle); 16: the bf16 kernels (emulating oracle)."""
    from nerf_meets_mlx_amd.models.NeRF import NeRF
    arch = O.NerfArch()
    kw = {} if precision is None else {"precision": precision}
    m = NeRF(channel_input=63, channel_input_views=27, is_use_view_directions=True, device=DEV, seed=seed, **kw)
    assert m.precision == (22 if precision is None else precision)
    p = O.init_params(arch, seed)
    flat = O.flatten_params(arch, p)
    assert torch.equal(m.params.cpu(), flat)             # same seeded init stream as the oracle
    if scale != 1.0:
        flat = flat * scale
        m.load_flat(flat)
    return m, arch, flat


@pytest.mark.parametrize("variant", [1, 2])
def test_mlp_forward_embedded_rows(variant):
    from nerf_meets_mlx_amd import _native
    _native.check(_native.lib().nerf_set_option(b"mlp_variant", variant))
    try:
        # weights x1.5: keeps activations O(1) through 8 layers so every layer matters in the comparison
        m, arch, flat = _model_pair(0, 1.5)
        p = O.unflatten_params(arch, flat)
        torch.manual_seed(5)
        for M in (1, 31, 32, 257, 4096):
            x = torch.randn(M, 90)
            got = m.forward(x.to(DEV)).cpu()
            emu = O.nerf_forward(arch, p, x, emulate_bf16=True)
            ref = O.nerf_forward(arch, p, x, emulate_bf16=False)
            assert got.shape == (M, 4)
            assert _relmax(got, emu) < 1e-2, (M, _relmax(got, emu))
            assert _relmax(got, ref) < 3e-2, (M, _relmax(got, ref))
    finally:
        _native.check(_native.lib().nerf_set_option(b"mlp_variant", 0))


def _rays(B, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * 4.0
    d = -o / 4.0 + 0.25 * torch.randn(B, 3, generator=g)
    return O.pack_rays(o, d, 2.0, 6.0)


@pytest.mark.parametrize("variant,quirk", [(1, True), (2, True), (2, False), (3, True), (3, False), (4, True), (4, False), (5, True), (5, False)])
def test_fused_query_matches_oracle(variant, quirk):
    from nerf_meets_mlx_amd import _native
    _native.check(_native.lib().nerf_set_option(b"mlp_variant", variant))
    try:
        m, arch, flat = _model_pair(1, 1.5)
        p = O.unflatten_params(arch, flat)
        for B, n in [(3, 64), (5, 192), (1, 7), (100, 64)]:
            rays = _rays(B, 10 + B)
            z = torch.sort(torch.rand(B, n) * 4 + 2, -1).values
            raw = m.query(rays.to(DEV), z.to(DEV), ref_quirks=quirk).cpu()
            o, d, _, _, vd = O.decompose_ray_batch(rays)
            pos = o[:, None, :] + z[:, :, None] * d[:, None, :]
            emu = O.run_model(arch, p, pos, vd, ref_quirks=quirk, emulate_bf16=True)
            ref = O.run_model(arch, p, pos, vd, ref_quirks=quirk, emulate_bf16=False)
            assert raw.shape == (B, n, 4)
            assert _relmax(raw, emu) < 1e-2, (B, n, _relmax(raw, emu))
            assert _relmax(raw, ref) < 3e-2, (B, n, _relmax(raw, ref))
    finally:
        _native.check(_native.lib().nerf_set_option(b"mlp_variant", 0))


def test_generic_query_path_and_rank_assert():
    from nerf_meets_mlx_amd.models import NeRF as NM, embedding
    m, arch, flat = _model_pair(2, 1.5, precision=None)                      # default precision: the float32 oracle at 1e-4
    fp, _ = embedding.get_embedder(10); fd, _ = embedding.get_embedder(4)
    q = NM.NetworkQuery(fp, fd, 1024)
    pos = torch.randn(4, 16, 3); vd = torch.nn.functional.normalize(torch.randn(4, 3), dim=-1)
    out = q(pos.to(DEV), vd.to(DEV), m).cpu()
    ref = O.run_model(arch, O.unflatten_params(arch, flat), pos, vd)
    assert out.shape == (4, 16, 4) and _relmax(out, ref) < 1e-4
    with pytest.raises(AssertionError):
        q(pos.reshape(-1, 3).to(DEV), vd.to(DEV), m)                         # models/NeRF.py:31
    bad = NM.NeRF(width_layers=128, channel_input=63, channel_input_views=27, is_use_view_directions=True, device=DEV, seed=0)
    with pytest.raises(ValueError):                                          # no HIP kernel, and no fallback
        bad.forward(torch.randn(8, 90, device=DEV))


def _rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("variant,B,n", [(1, 6, 40), (2, 6, 40), (3, 6, 40), (2, 64, 96), (3, 64, 96), (3, 300, 64)])
def test_mlp_backward_matches_autograd(variant, B, n):
    """dW/db of the HIP backward vs torch autograd through the bf16-emulating oracle.
    The HIP chain also rounds every dZ_l to bf16 and units whose pre-activation is ~0 can take the
    other ReLU branch (forward values differ in the last bf16 bit), so single entries move by a few
    percent of the tensor's max; the tensor as a whole must agree: rel-L2 < 3e-2 (6e-2 for the 240-sample
    case), rel-max < 4x that."""
    from nerf_meets_mlx_amd import _native
    _native.check(_native.lib().nerf_set_option(b"mlp_variant", variant))
    try:
        m, arch, flat = _model_pair(3, 1.5)
        torch.manual_seed(1000 * B + n)
        rays = _rays(B, 77)                                  # (6,40): 240 samples = 7.5 fragment tiles (ragged tail)
        z = torch.sort(torch.rand(B, n) * 4 + 2, -1).values
        raw = m.query(rays.to(DEV), z.to(DEV), train=True)
        g = torch.randn(B, n, 4)
        grads = m.backward(g.to(DEV)).cpu()
        fl = flat.clone().requires_grad_(True)
        o, d, _, _, vd = O.decompose_ray_batch(rays)
        pos = o[:, None, :] + z[:, :, None] * d[:, None, :]
        out = O.run_model(arch, O.unflatten_params(arch, fl), pos, vd, emulate_bf16=True)
        (out * g).sum().backward()
        want = fl.grad
        assert _relmax(raw.cpu(), out.detach()) < 1e-2
        tol = 6e-2 if B * n < 1000 else 3e-2      # rounding / ReLU-flip noise averages out as 1/sqrt(samples);
        # measured 1.2-2.1e-2 on the deepest tensors (pos0, pos3) over seeds, so 2e-2 was a coin flip
        off = 0
        for name, o_, i_ in arch.layer_shapes():
            for part, cnt in (("W", o_ * i_), ("b", o_)):
                a, b = grads[off:off + cnt], want[off:off + cnt]
                assert _rel_l2(a, b) < tol and _relmax(a, b) < 4 * tol, (name, part, _rel_l2(a, b), _relmax(a, b))
                off += cnt
        assert off == 595844
        assert _rel_l2(grads, want) < tol / 2
    finally:
        _native.check(_native.lib().nerf_set_option(b"mlp_variant", 0))


def test_adam_matches_oracle():
    from nerf_meets_mlx_amd.models.NeRF import Adam
    m, arch, flat = _model_pair(4)
    opt = Adam(5e-4, shared_state=True)
    p = flat.clone(); mm = torch.zeros_like(p); vv = torch.zeros_like(p)
    torch.manual_seed(9)
    for step in range(3):
        g = torch.randn_like(p) * 1e-3
        m.grads.copy_(g.to(DEV))
        opt.update(m)
        O.adam_step(p, g, mm, vv, 5e-4)
        np.testing.assert_allclose(m.params.cpu().numpy(), p.numpy(), rtol=0, atol=3e-7)
    opt2 = Adam(1e-3, bias_correction=True, shared_state=False)
    p2 = flat.clone(); m2 = torch.zeros_like(p2); v2 = torch.zeros_like(p2)
    m.load_flat(flat)
    for step in range(1, 3):
        g = torch.randn_like(p2) * 1e-3
        opt2.update(m, g.to(DEV))
        O.adam_step(p2, g, m2, v2, 1e-3, bias_correction=True, step=step)
        np.testing.assert_allclose(m.params.cpu().numpy(), p2.numpy(), rtol=0, atol=3e-6)


# ------------------------------------------------------------------------------ a14 / a18 / a19
@pytest.mark.parametrize("precision", [None, 16])
def test_render_rays_eval_end_to_end(precision):
    """precision None = the default (22): against the FLOAT32 oracle, rgb to 1e-3 (the importance samples of a ray move with
    its coarse weights; raw itself is at 1e-5); 16: against the bf16-emulating oracle at the bf16 bars."""
    from nerf_meets_mlx_amd.rendering import render
    from nerf_meets_mlx_amd.models import NeRF as NM, embedding
    mc, arch, fc = _model_pair(5, 1.5, precision)
    mf, _, ff = _model_pair(6, 1.5, precision)
    emu = precision == 16
    tc, tf = (2e-2, 3e-2) if emu else (1e-3, 1e-3)
    fp, _ = embedding.get_embedder(10); fd, _ = embedding.get_embedder(4)
    q = NM.NetworkQuery(fp, fd, 65536)
    B, n, Nn = 48, 64, 128
    rays = _rays(B, 3)
    u = torch.rand(B, Nn)
    got = render.render_rays_eval(rays.to(DEV), mc, q, n, N_importance=Nn, network_fine=mf, white_bkgd=True, u=u.to(DEV))
    want = O.render_rays_eval(arch, O.unflatten_params(arch, fc), O.unflatten_params(arch, ff), rays, n, Nn, u,
                              white_bkgd=True, emulate_bf16=emu)
    assert set(got) >= {"rgb_map", "disp_map", "acc_map", "rgb_coarse", "disp_coarse", "acc_coarse", "z_vals", "weights"}
    assert got["weights"].shape == (B, n, 1) and got["z_vals"].shape == (B, n)
    assert torch.equal(got["z_vals"].cpu(), want["z_vals"])
    np.testing.assert_allclose(got["rgb_coarse"].cpu().numpy(), want["rgb_coarse"].numpy(), atol=tc)
    np.testing.assert_allclose(got["rgb_map"].cpu().numpy(), want["rgb_map"].numpy(), atol=tf)
    cg = render.render_rays(rays.to(DEV), mc, q, n, white_bkgd=True, N_importance=Nn, network_fine=mf)
    assert torch.equal(cg["rgb_map"], cg["rgb_coarse"])                      # coarse-only (:112-162)


@pytest.mark.parametrize("precision", [None, 16])
def test_render_full_frame_small(precision):
    from nerf_meets_mlx_amd.rendering import render
    from nerf_meets_mlx_amd.models import NeRF as NM, embedding
    mc, arch, fc = _model_pair(7, 1.5, precision)
    emu = precision == 16
    tol = 3e-2 if emu else 1e-3
    fp, _ = embedding.get_embedder(10); fd, _ = embedding.get_embedder(4)
    H = W = 12
    K = _lego_K(H, W)
    c2w = O.pose_spherical(30.0, -30.0, 4.0)[:3, :4]
    u = torch.rand(H * W, 16)
    kw = dict(network_coarse=mc, network_fine=None, network_query_fn=NM.NetworkQuery(fp, fd, 65536), n_depth_samples=32,
              N_importance=16, white_bkgd=True, render_rays_func=render.render_rays_eval, use_viewdirs=True, ndc=False,
              near=2.0, far=6.0, u=u.to(DEV))
    rgb, disp, acc, extras = render.render(H, W, K, chunk=50, c2w=c2w, **kw)
    w_rgb, w_disp, w_acc, w_ex = O.render(arch, O.unflatten_params(arch, fc), None, H, W, K, c2w, 2.0, 6.0, 32, 16, u,
                                          chunk=50, white_bkgd=True, emulate_bf16=emu)
    assert rgb.shape == (H, W, 3) and disp.shape == (H, W, 1) and acc.shape == (H, W, 1)
    assert extras["z_vals"].shape == (H, W, 32) and extras["weights"].shape == (H, W, 32, 1)
    np.testing.assert_allclose(rgb.cpu().numpy(), w_rgb.numpy(), atol=tol)
    np.testing.assert_allclose(acc.cpu().numpy(), w_acc.numpy(), atol=tol)


# ------------------------------------------------------------------------------ engine (8f-1)
@pytest.mark.parametrize("precision", [None, 16])
def test_trainer_matches_oracle_trainer(precision):
    """Same rays / targets / uniforms through the HIP Trainer and the OracleTrainer (fp32 autograd): the per-iteration
    losses of the reference loop ordering must track.  Default precision (22): 1e-3 for the first two iterations, 2 % for
    the next two (Adam's first steps are lr * sign(g): trajectories separate at parameters whose gradient is ~0, whatever the
    arithmetic); precision 16 (bf16): 3 % / 12 %."""
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    H = W = 8
    imgs = torch.rand(2, H, W, 3)
    poses = torch.stack([O.pose_spherical(10.0, -30.0, 4.0), O.pose_spherical(100.0, -40.0, 4.0)])
    kw = {} if precision is None else {"precision": precision}
    tr = Trainer(imgs, poses, _lego_K(H, W), N_rand=48, n_depth_samples=64, N_importance=128, seed=11, device=DEV, **kw)
    assert tr.coarse.precision == (22 if precision is None else 16)
    ot = O.OracleTrainer(O.NerfArch(), 64, 128, seed=11)
    assert torch.equal(tr.coarse.params.cpu(), ot.pc.detach()) and torch.equal(tr.fine.params.cpu(), ot.pf.detach())
    g = torch.Generator().manual_seed(5)
    for it in range(4):
        rays, target = tr.sample_batch()
        u = torch.rand(48, 128, generator=g)
        got = tr.train_step(rays, target, u.to(DEV))
        want = ot.step(rays[:, 0:3].cpu(), rays[:, 3:6].cpu(), target.cpu(), u)
        for k in ("loss_coarse", "loss_fine"):
            # Adam's first updates are ~lr*sign(g): sign flips of tiny gradients make the two
            # trajectories drift apart step by step (bf16 vs fp32), so the band widens with `it`
            tol = (3e-2 if it < 2 else 1.2e-1) if precision == 16 else (1e-3 if it < 2 else 2e-2)
            assert abs(float(got[k]) - want[k]) < tol * abs(want[k]) + 1e-5, (it, k, float(got[k]), want[k])
        assert abs(tr.opt.learning_rate * 0.1 ** (1 / 500000) - ot.lr) < 1e-9
    assert len(tr.opt.state) == 1                                  # Q7: one shared (m, v)
    # parameters moved together: Adam's first steps are ~lr * sign(g); compare where |g| is not tiny
    dp = (tr.coarse.params.cpu() - ot.pc.detach()).abs()
    assert float(dp.mean()) < 6e-4                                 # < 10 % of the 4 x lr*3.16 a parameter can travel
    sd = tr.state_dict()
    tr2 = Trainer(imgs, poses, _lego_K(H, W), N_rand=48, seed=99, device=DEV, **kw)
    tr2.load_state_dict(sd)
    assert torch.equal(tr2.coarse.params, tr.coarse.params) and tr2.it == 4 and tr2.seed == 11      # continues the saved run's streams
    ra, _ = tr.sample_batch(); rb, _ = tr2.sample_batch()
    assert torch.equal(ra, rb)
    img = tr.render_frame(poses[0])
    assert img.shape == (H, W, 3) and torch.isfinite(img).all()


# ------------------------------------------------------------------------------ config 1 / 8f-4: image fitting
def test_image_model_forward_backward():
    """The no-view-direction model of the image-learning entrypoint (40 -> 8x256 skip 4 -> 3) in the bf16 mode (precision=16,
    declared reduced precision); the reference-tolerance modes of the same model: tests/test_gpu_round5.py."""
    from nerf_meets_mlx_amd.models.NeRF import NeRF
    arch = O.NerfArch(channel_input=40, channel_input_views=0, channel_output=3, use_viewdirs=False)
    m = NeRF(channel_input=40, channel_input_views=0, channel_output=3, is_use_view_directions=False, device=DEV, seed=0,
             precision=16)
    assert m.n_params == 482051
    flat = O.flatten_params(arch, O.init_params(arch, 0)) * 1.5
    m.load_flat(flat)
    torch.manual_seed(11)
    for M in (1, 33, 2500):
        x = torch.randn(M, 40)
        got = m.forward(x.to(DEV)).cpu()
        p = O.unflatten_params(arch, flat)
        assert got.shape == (M, 3)
        assert _relmax(got, O.nerf_forward(arch, p, x, emulate_bf16=True)) < 1e-2
        assert _relmax(got, O.nerf_forward(arch, p, x)) < 3e-2
    x = torch.randn(2500, 40); g = torch.randn(2500, 3)
    out = m.forward(x.to(DEV), train=True)
    grads = m.backward(g.to(DEV)).cpu()
    fl = flat.clone().requires_grad_(True)
    (O.nerf_forward(arch, O.unflatten_params(arch, fl), x, emulate_bf16=True) * g).sum().backward()
    off = 0
    for name, o_, i_ in arch.layer_shapes():
        for part, cnt in (("W", o_ * i_), ("b", o_)):
            a, b = grads[off:off + cnt], fl.grad[off:off + cnt]
            # single entries move with ReLU flips of near-zero units (see test_mlp_backward_matches_autograd)
            assert _rel_l2(a, b) < 2e-2 and _relmax(a, b) < 1.2e-1, (name, part, _rel_l2(a, b), _relmax(a, b))
            off += cnt
    assert off == 482051


# ------------------------------------------------------------------------------ configs[4]: Instant-NGP-sized model
def _small_pair(scale=1.5):
    from nerf_meets_mlx_amd.models.NeRF import NeRF
    arch = O.NerfArch(channel_input=32, channel_input_views=16, n_layers=2, width=64, skips=(), use_viewdirs=True)
    m = NeRF(n_layers=2, width_layers=64, channel_input=32, channel_input_views=16, list_skip_connection_layers=[],
             is_use_view_directions=True, device=DEV, seed=0, precision=16)        # bf16 mode; precision 22: test_gpu_round5.py
    assert m.n_params == 13188 == arch.n_params()
    flat = O.flatten_params(arch, O.init_params(arch, 0)) * scale
    m.load_flat(flat)
    return m, arch, flat


def test_small_model_forward_backward_and_input_grads():
    """NeRF(n_layers=2, width=64, in 32+16, view head): forward, dW/db and dL/d(position features) vs autograd
    through the bf16-emulating oracle (ragged M: 1, 33, 4100 samples)."""
    m, arch, flat = _small_pair()
    p = O.unflatten_params(arch, flat)
    torch.manual_seed(21)
    for M in (1, 33, 4100):
        x = torch.randn(M, 48)
        got = m.forward(x.to(DEV)).cpu()
        assert got.shape == (M, 4)
        assert _relmax(got, O.nerf_forward(arch, p, x, emulate_bf16=True)) < 1e-2
        assert _relmax(got, O.nerf_forward(arch, p, x)) < 3e-2
    M = 4100
    x = torch.randn(M, 48); g = torch.randn(M, 4)
    out = m.forward(x.to(DEV), train=True)
    grads, d_x = m.backward(g.to(DEV), need_input_grad=True)
    grads, d_x = grads.cpu(), d_x.cpu()
    fl = flat.clone().requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    want_out = O.nerf_forward(arch, O.unflatten_params(arch, fl), xr, emulate_bf16=True)
    (want_out * g).sum().backward()
    assert _relmax(out.cpu(), want_out.detach()) < 1e-2
    off = 0
    for name, o_, i_ in arch.layer_shapes():
        for part, cnt in (("W", o_ * i_), ("b", o_)):
            a, b = grads[off:off + cnt], fl.grad[off:off + cnt]
            assert _rel_l2(a, b) < 2e-2 and _relmax(a, b) < 1.2e-1, (name, part, _rel_l2(a, b), _relmax(a, b))
            off += cnt
    assert off == 13188
    assert d_x.shape == (M, 32)
    assert _rel_l2(d_x, xr.grad[:, :32]) < 2e-2, _rel_l2(d_x, xr.grad[:, :32])
    # the gradient without input grads is the same parameter gradient
    m.forward(x.to(DEV), train=True)
    assert torch.equal(m.backward(g.to(DEV)).cpu(), grads) or _rel_l2(m.grads.cpu(), grads) < 1e-5


@pytest.mark.parametrize("half_tables", [False, True])
def test_ngp_field_gradients_and_training_track_oracle(half_tables):
    """configs[4] in the bf16 mode (precision=16, declared reduced precision; the default precision 22 against the float32
    oracle: tests/test_gpu_round5.py): hash grid (small tables so that autograd on the oracle is cheap) + SH + 2 x 64 MLP.  One batch:
    loss, MLP gradient and table gradient vs autograd through the bf16-emulating oracle; then 6 Adam iterations on
    identical batches: losses track and fall.  half_tables (round 4, the default): the fused query gathers from the fp16 shadow
    image of the tables -- same bars against the oracle; the fused == unfused BIT equality holds for float32 gathers only."""
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    from nerf_meets_mlx_amd.dataset import synthetic
    H = W = 32
    imgs, poses, _, hwf, K = synthetic.make_dataset(H, W, 2, seed=0, device=DEV)
    kw = dict(n_levels=16, min_res=4, max_res=128, n_features_per_level=2, log2_hashmap_size=12, hash_init_scale=0.5)
    tr = NGPTrainer(imgs, poses, K, N_rand=256, n_depth_samples=32, seed=0, device=DEV, half_tables=half_tables, precision=16, **kw)
    orc = O.OracleNGP(tr.field.enc.tables.cpu(), tr.field.enc.scaled_res, seed=0, n_samples=32, emulate_bf16=True)
    assert torch.equal(tr.field.mlp.params.cpu(), orc.p.detach())
    # The seed-0 network is DEAD at initialisation (sigma in [-0.22, -0.10] on every sample -> all weights 0, rgb = white,
    # every gradient exactly 0: DESIGN.md section 7) -- found in round 5: the gradient bars below were met by 0 == 0.  Lift the
    # alpha bias (flat index 10496) on both sides so that the comparison is about a live network.
    with torch.no_grad():
        orc.p[10496] += 0.6
    tr.field.mlp.load_flat(orc.p.detach())
    rays, target = tr.sample_batch()
    ro, rd, tg = rays[:, 0:3].cpu(), rays[:, 3:6].cpu(), target.cpu()
    # --- fused row encoder == stand-alone encoders, bit for bit
    from nerf_meets_mlx_amd import sampling
    z0 = sampling.sample_coarse(rays, 32)
    pa, xa = tr.field.features(rays, z0)
    pb, xb = tr.field.features_unfused(rays, z0)
    assert torch.equal(pa, pb) and torch.equal(xa, xb)
    # --- rows computed inside the forward kernel == rows through HBM (same bf16 fragments, same MFMAs), and the
    # --- table gradient from rays == the table gradient from the point list
    raw_f = tr.field.query(rays, z0, train=True, fused=True)
    g0 = torch.randn_like(raw_f)
    gm_f, _ = tr.field.backward(g0); gm_f, gt_f = gm_f.clone(), tr.field.table_grad().clone()
    raw_u = tr.field.query(rays, z0, train=True, fused=False)
    gm_u, _ = tr.field.backward(g0); gt_u = tr.field.table_grad()
    if half_tables:      # fp16 table values (2^-11) under the bf16 rounding of the interpolated features (2^-9)
        assert float((raw_f - raw_u).abs().max()) < 5e-3 * float(raw_u.abs().max())
        assert _rel_l2(gm_f.cpu(), gm_u.cpu()) < 2e-2 and _rel_l2(gt_f.cpu(), gt_u.cpu()) < 2e-2
    else:
        assert torch.equal(raw_f, raw_u)
        assert _rel_l2(gm_f.cpu(), gm_u.cpu()) < 1e-5 and _rel_l2(gt_f.cpu(), gt_u.cpu()) < 1e-5    # atomics: order only
    # --- gradients of one batch (no update)
    from nerf_meets_mlx_amd.rendering import render
    from nerf_meets_mlx_amd.ops.metric import mse_loss_grad
    z = sampling.sample_coarse(rays, 32)
    raw = tr.field.query(rays, z, train=True)
    rgb = render.composite(raw, z, rays, 0.0, True)[0]
    loss, d_rgb = mse_loss_grad(rgb, target)
    g_mlp, _ = tr.field.backward(render.composite_backward(raw, z, rays, d_rgb, True)); g_tab = tr.field.table_grad()
    lo, gp, gt = orc.loss_and_grads(ro, rd, tg)
    assert float(gp.norm()) > 1e-3 and float(gt.norm()) > 1e-4, "dead network: the comparison would be 0 == 0"
    assert abs(float(loss) - float(lo)) < 2e-2 * float(lo), (float(loss), float(lo))
    assert _rel_l2(g_mlp.cpu(), gp) < 5e-2, _rel_l2(g_mlp.cpu(), gp)
    assert _rel_l2(g_tab.cpu(), gt) < 5e-2, _rel_l2(g_tab.cpu(), gt)
    # --- a few iterations on identical batches
    hip, ora = [], []
    for it in range(6):
        rays, target = tr.sample_batch()
        hip.append(float(tr.train_step(rays, target)["loss_coarse"]))
        ora.append(orc.step(rays[:, 0:3].cpu(), rays[:, 3:6].cpu(), target.cpu()))
    for a, b in zip(hip[:2], ora[:2]):
        assert abs(a - b) < 5e-2 * b, (hip, ora)
    for a, b in zip(hip, ora):
        assert abs(a - b) < 0.25 * b, (hip, ora)
    fixed = [float(tr.train_step(rays, target)["loss_coarse"]) for _ in range(8)]      # the SAME batch eight times: the loss falls
    assert fixed[-1] < fixed[0], fixed
    img = tr.render_frame(poses[0], shard=False)
    assert img.shape == (H, W, 3) and torch.isfinite(img).all()


def test_input_grads_refused_for_the_large_models():
    from nerf_meets_mlx_amd.models.NeRF import NeRF
    m = NeRF(channel_input=63, channel_input_views=27, is_use_view_directions=True, device=DEV, seed=0)
    x = torch.randn(64, 90, device=DEV)
    m.forward(x, train=True)
    with pytest.raises((RuntimeError, ValueError)):
        m.backward(torch.randn(64, 4, device=DEV), need_input_grad=True)


def test_image_fitter_tracks_oracle_loop():
    """entrypoints/__viser_image_learning.py loop, headless, in the bf16 mode (precision=16; the default precision against
    the float32 oracle loop at float32-class bars: tests/test_gpu_round5.py): same integer-coordinate batches through the HIP
    ImageFitter and the oracle loop; losses track (3 % for 2 steps, 12 % for the next 4) and the fit improves."""
    from nerf_meets_mlx_amd.entrypoints.image_learning import ImageFitter
    torch.manual_seed(3)
    H = W = 40
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    img = torch.stack([0.5 + 0.5 * torch.sin(6 * xx), yy, 0.5 + 0.5 * torch.cos(5 * (xx + yy))], -1)
    fit = ImageFitter(img.to(DEV), batch_downsample_factor=4, seed=0, precision=16)
    orc = O.OracleImageFitter(seed=0)
    assert torch.equal(fit.model.params.cpu(), orc.p.detach())
    assert fit.batch == 400 and fit.embed.get_out_dim() == 40
    losses = []
    it = 0
    for epoch in range(2):
        for X, y in fit.batch_iterate():
            assert X.shape == (400, 2) and torch.equal(X, X.round())          # integer (row, col) coordinates
            lh = float(fit.step(X, y))
            lo, _ = orc.step(X.cpu(), y.cpu())
            tol = 3e-2 if it < 2 else 1.2e-1
            if it < 6:
                assert abs(lh - lo) < tol * lo + 1e-6, (it, lh, lo)
            losses.append(lh)
            it += 1
        fit.epoch += 1
    assert losses[-1] < 0.5 * losses[0]
    pred = fit.predict()
    assert pred.shape == (H, W, 3) and torch.isfinite(pred).all()


# ------------------------------------------------------------------------------ fused renderer entry point
def test_render_rays_fused_equals_staged_path():
    """nerf_render_rays_fused enqueues the same kernels as render_rays_eval: results must be bit-identical."""
    from nerf_meets_mlx_amd.rendering import render
    from nerf_meets_mlx_amd.models import NeRF as NM, embedding
    mc, arch, fc = _model_pair(5, 1.5, precision=None)
    mf, _, ff = _model_pair(6, 1.5, precision=None)
    fp, _ = embedding.get_embedder(10); fd, _ = embedding.get_embedder(4)
    q = NM.NetworkQuery(fp, fd, 65536)
    B, n, Nn = 300, 64, 128
    rays = _rays(B, 3).to(DEV)
    u = torch.rand(B, Nn, device=DEV)
    a = render.render_rays_eval(rays, mc, q, n, N_importance=Nn, network_fine=mf, white_bkgd=True, u=u)
    b = render.render_rays_fused(rays, mc, mf, n, Nn, u=u, white_bkgd=True)
    for k in ("rgb_map", "disp_map", "acc_map", "rgb_coarse", "acc_coarse", "z_vals", "weights"):
        assert torch.equal(a[k], b[k]), k
    c = render.render_rays_fused(rays, mc, None, n, 0, white_bkgd=False)
    d = render.render_rays(rays, mc, q, n, white_bkgd=False)
    assert torch.equal(c["rgb_map"], d["rgb_map"]) and torch.equal(c["weights"], d["weights"])


def test_native_rccl_allreduce_single_rank():
    """nerf_comm_* / nerf_allreduce_grads (RCCL resolved lazily): a 1-rank communicator is the identity."""
    from nerf_meets_mlx_amd import parallel
    comm = parallel.NativeComm(0, 1, DEV)
    g = torch.randn(595844, device=DEV)
    want = g.clone()
    comm.allreduce_sum_(g)
    torch.cuda.synchronize()
    assert torch.equal(g, want)
    comm.close()


def test_headless_entrypoint_runs(tmp_path):
    """entrypoints/__test_nerf.py:main without the GUI: a few iterations on the synthetic scene (its run log goes under
    tmp_path, not the working directory)."""
    from nerf_meets_mlx_amd.entrypoints import test_nerf
    res = test_nerf.main(None, max_iter=3, hw_synthetic=32, n_train_synthetic=2, render_every=3, n_render_poses=1,
                         log_every=1, argv=["--basedir", str(tmp_path)])
    assert len(res["losses"]) == 3 and all(np.isfinite(l[1]) and np.isfinite(l[2]) for l in res["losses"])
    assert res["frames"][0].shape == (32, 32, 3) and res["video"][0].shape == (32, 32, 3)
    assert res["trainer"].it == 3


def test_streams_empty_and_ragged_inputs():
    """Launches go to the caller's stream; empty batches are no-ops; ragged sizes (M % 32 != 0, B not a multiple of
    the 8-tile super-tile) never touch memory outside their buffers (outputs compared with a padded run)."""
    from nerf_meets_mlx_amd import sampling
    from nerf_meets_mlx_amd.rendering import render
    m, arch, flat = _model_pair(8, 1.5, precision=None)
    rays = _rays(77, 21).to(DEV)
    z = sampling.sample_coarse(rays, 19)                                    # 1463 samples = 45.7 tiles
    ref = m.query(rays, z)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        on_side = m.query(rays, z)
        rgb_side = render.composite(on_side, z, rays, 0.0, True)[0]
    s.synchronize()
    assert torch.equal(on_side, ref)
    assert torch.equal(rgb_side, render.composite(ref, z, rays, 0.0, True)[0])
    # a prefix of the batch gives the prefix of the result (no cross-talk between tiles)
    assert torch.equal(m.query(rays[:5].contiguous(), z[:5].contiguous()), ref[:5])
    # empty batch
    e = m.query(rays[:0].contiguous(), z[:0].contiguous())
    assert e.shape == (0, 19, 4)
    assert sampling.sample_coarse(rays[:0].contiguous(), 8).shape == (0, 8)
    zn, zm = sampling.importance_sample(z[:0].contiguous(), torch.zeros(0, 19, device=DEV), 4, u=torch.zeros(0, 4, device=DEV))
    assert zn.shape == (0, 4) and zm.shape == (0, 23)
    # guard bytes around the outputs stay untouched
    buf = torch.full((77 * 19 * 4 + 64,), 7.0, device=DEV)
    out = buf[32:32 + 77 * 19 * 4].view(77, 19, 4)
    import ctypes as C
    from nerf_meets_mlx_amd import _native as N
    N.check(N.lib().nerf_query_fused(C.byref(m.arch), N.ptr(m.packed()), N.ptr(rays), N.ptr(z), 77, 19, 0,
                                     C.c_void_p(out.data_ptr()), None, N.stream()))
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and bool((buf[:32] == 7.0).all()) and bool((buf[-32:] == 7.0).all())


def test_render_rays_perturb_lindisp_and_noise_paths():
    """The options the reference's train kwargs carry (perturb, raw_noise_std, lindisp, retraw) through render_rays."""
    from nerf_meets_mlx_amd.rendering import render
    from nerf_meets_mlx_amd.models import NeRF as NM, embedding
    mc, arch, fc = _model_pair(9, 1.5, precision=None)
    fp, _ = embedding.get_embedder(10); fd, _ = embedding.get_embedder(4)
    q = NM.NetworkQuery(fp, fd, 65536)
    rays = _rays(40, 31).to(DEV)
    torch.manual_seed(0)
    base = render.render_rays(rays, mc, q, 32, white_bkgd=True, retraw=True)
    assert base["raw"].shape == (40, 32, 4)
    jit = render.render_rays(rays, mc, q, 32, white_bkgd=True, perturb=1.0)
    z0, z1 = base["z_vals"], jit["z_vals"]
    assert not torch.equal(z0, z1) and bool((z1[:, 1:] >= z1[:, :-1]).all())
    mids = 0.5 * (z0[:, 1:] + z0[:, :-1])
    assert bool((z1[:, 1:-1] >= mids[:, :-1] - 1e-5).all()) and bool((z1[:, 1:-1] <= mids[:, 1:] + 1e-5).all())
    noisy = render.render_rays(rays, mc, q, 32, white_bkgd=True, raw_noise_std=1.0)
    assert torch.isfinite(noisy["rgb_map"]).all() and not torch.equal(noisy["rgb_map"], base["rgb_map"])
    ld = render.render_rays(rays, mc, q, 32, white_bkgd=True, lindisp=True)
    assert float(ld["z_vals"][0, 0]) == 0.0                                   # literal formula, Q12
    # oracle cross-check of the jittered pass with the same uniforms
    from nerf_meets_mlx_amd import sampling
    t = torch.rand(40, 32)
    zg = sampling.sample_coarse(rays, 32, perturb=1.0, t_rand=t.to(DEV)).cpu()
    r = rays.cpu()
    want = O.add_noise_z(O.sample_z_uniform(r[:, 6:7], r[:, 7:8], 32), 1.0, t)
    np.testing.assert_allclose(zg.numpy(), want.numpy(), atol=1e-6)


def test_autograd_wrappers_match_explicit_backward():
    """loss.backward() through autograd.FusedQuery / Composite == the explicit kernel sequence of the Trainer."""
    from nerf_meets_mlx_amd import autograd as AG, sampling
    from nerf_meets_mlx_amd.models.NeRF import Adam
    from nerf_meets_mlx_amd.ops.metric import mse_loss_grad
    from nerf_meets_mlx_amd.rendering import render
    m, arch, flat = _model_pair(4, 1.0, precision=None)
    rays = _rays(50, 5).to(DEV)
    y = torch.rand(50, 3, device=DEV)
    out = AG.render_rays_grad(rays, m, 64, white_bkgd=True)
    loss = ((out["rgb_map"] - y) ** 2).mean() + 0.1 * out["acc_map"].mean() + 0.01 * out["depth_map"].mean()
    loss.backward()
    g_auto = m.params.grad.clone()
    # explicit path
    z = sampling.sample_coarse(rays, 64)
    raw = m.query(rays, z, train=True)
    rgb, _, acc, _, depth = render.composite(raw, z, rays, 0.0, True)
    _, d_rgb = mse_loss_grad(rgb, y)
    d_acc = torch.full((50,), 0.1 / 50, device=DEV); d_dep = torch.full((50,), 0.01 / 50, device=DEV)
    g_exp = m.backward(render.composite_backward(raw, z, rays, d_rgb, True, d_acc, d_dep)).clone()
    assert _rel_l2(g_auto.cpu(), g_exp.cpu()) < 1e-5              # same kernels; only float atomics order differs
    assert float(g_auto.abs().max()) > 0
    Adam(5e-4).update(m, g_auto)                                    # in-place update of the leaf works
    assert not torch.equal(m.params.detach().cpu(), flat)


# ------------------------------------------------------------------------------ bench.py contract
@pytest.mark.parametrize("extra", [["--full"], ["--full", "--config", "ngp"], ["--full", "--n-importance", "0"], [], ["--config", "ngp"]])
def test_bench_prints_one_contract_json_line(extra):
    """bench.py (small sizes, child process): exactly one JSON line with the driver's keys, a roofline object, finite
    positive numbers; the legs beside the headline come with --full only (the cpu_baseline leg, >= 10 s of CPU work, is
    exercised by the full-size run only), and a plain run carries none of them."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    full = "--full" in extra
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--n-rand", "256",
           "--render-rays", "2048", "--hw", "64"] + (["--no-cpu-baseline", "--sustain-seconds", "1", "--fp32-steps", "2"] if full else []) + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["unit"] == "rays/s" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 0 and np.isfinite(d["value"]) and d["ms_per_step"] > 0
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["achieved"] > 0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert abs(d["value"] - (256 + 2048) * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
    if not full:
        for leg in ("sustained", "lego_batch", "fp32", "bf16", "f32tol", "reference_precision_value", "frame", "ngp", "cpu_baseline"):
            assert leg not in d, leg
    elif "--config" not in extra:
        # the legs the --full N = 1 line carries beside the contract keys (round 3): the same step sustained, at the
        # reference's arithmetic (fp32 models), at lego.txt's batch, and the configs[4] step
        for leg in ("sustained", "fp32", "lego_batch", "ngp"):
            assert leg in d and d[leg]["value"] > 0 and np.isfinite(d[leg]["value"]), leg
        assert d["sustained"]["seconds"] >= 1.0 and 0.3 < d["sustained"]["ratio_to_burst"] < 3.0
        assert d["fp32"]["dtype"] == "f32" and d["fp32"]["roofline"]["peak"] == 157.3 and d["fp32"]["value"] < d["value"]
        assert d["lego_batch"]["n_rand_per_gpu"] == 1024 and "roofline" in d["ngp"]
        # round 5: the label names the OPERANDS (two 16-bit numbers per float32 value), and configs[4]'s value is the
        # reference-tolerance mode with the bf16 mode as a declared extra leg
        assert not d["dtype"].startswith("f32") and d["operand_significand_bits"] == {"render": 22, "train": 16}
        assert d["ngp"]["dtype"].startswith("split16") and d["ngp"]["bf16"]["value"] > 0 and d["ngp"]["bf16"]["dtype"].startswith("bf16")
    if "--config" in extra:
        assert d["config"]["precision"] == 22 and d["dtype"].startswith("split16") and (not full or d["bf16"]["value"] > 0)
    assert d["rank_ms_per_step"] is None                                   # N = 1


@pytest.mark.parametrize("extra", [[], ["--config", "ngp"]])
def test_bench_dump_outputs_are_reproducible(extra, tmp_path):
    """--dump-outputs DIR: the last timed step's render rgb, losses and parameters as float32 .npy (hash tables as a seeded
    sample), 64 MB at most; two runs with the same arguments write the same arrays (losses: up to float-atomic rounding),
    and --steps is the number of timed steps (a third run with one more step leaves different parameters)."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for run, steps in enumerate((3, 3, 4)):
        d = tmp_path / f"run{run}"
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--steps", str(steps), "--warmup", "1", "--n-rand", "256",
               "--render-rays", "2048", "--hw", "64", "--no-cpu-baseline", "--no-extra-legs", "--dump-outputs", str(d)] + extra
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads([l for l in out.stdout.splitlines() if l.strip()][-1])
        assert line["steps"] == steps and line["ms_per_step"] > 0
        files = sorted(os.listdir(d))
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        dumps.append({f[:-4]: np.load(d / f) for f in files})
    a, b, c = dumps
    want = {"render_rgb", "loss_coarse"} | ({"tables_params_sample", "mlp_params"} if extra else {"loss_fine", "coarse_params", "fine_params"})
    assert set(a) == want, sorted(a)
    assert a["render_rgb"].shape == (2048, 3)
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all(), k
        if k.startswith("loss"):            # summed with float atomics (composite.hip): order-dependent in the last bits
            np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=0, err_msg=k)
        else:
            assert np.array_equal(a[k], b[k]), k
    # one more timed step: different parameters after it
    key = "mlp_params" if extra else "coarse_params"
    assert not np.array_equal(a[key], c[key])
