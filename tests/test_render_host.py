"""CPU-only checks of tests/_render_ref.py, the float32 emulation the GPU tests hold csrc/sampling.hip and csrc/composite.hip to.

The emulation is tied to the float64 oracle (not to the kernels) by forward-error bounds of float32 arithmetic: with
gamma_k = k u / (1 - k u), u = 2^-24, a length-n float32 sum errs by at most gamma_n sum|x|.  Inputs keep the float32 exponent
finite (negative prefix above -80, x below 80 except the 1e10 last interval whose exp(-x) is 0 in both); that domain is asserted
on the inputs.  Also here: the merge rule with a transcription of the kernel's two merge branches, and the argument checks of
the seven entry points.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import _render_ref as R

f32 = np.float32
E = 2.0
T64 = lambda a: torch.from_numpy(np.asarray(a)).double()


def _inputs(B, n, seed):
    rng = np.random.default_rng(seed)
    z = np.sort(rng.random((B, n), dtype=f32) * 4 + 2, -1)
    raw = rng.standard_normal((B, n, 4)).astype(f32)
    raw[..., 3] = np.clip(raw[..., 3] * 3, -0.5, 50)
    d = rng.standard_normal((B, 3)).astype(f32)
    x = (np.diff(z.astype(np.float64), axis=-1) * np.linalg.norm(d.astype(np.float64), axis=-1)[:, None]) * raw[:, :-1, 3]
    if n > 1:                                             # the domain: float32 exponents stay finite
        cs = np.cumsum(x, -1)
        assert cs.min() > -80 and x.max() < 80
    return raw, z, d, rng


@pytest.mark.parametrize("n", [1, 2, 64, 65, 193, 300, 1024])
@pytest.mark.parametrize("white", [False, True])
def test_forward_emulation_against_float64_oracle(n, white):
    B = 9
    raw, z, d, _ = _inputs(B, n, n)
    rgb, disp, acc, w, depth = R.composite_forward(raw, z, d, white, E=E)
    o_rgb, o_disp, o_acc, o_w, o_depth = (t.numpy() for t in O.raw2outputs(T64(raw), T64(z), T64(d), 0.0, white))
    o_w = o_w[..., 0]
    # exponent: |S32 - S64| <= gamma_(n+7) sum|x| (7 scan levels + lane prefix <= n additions, + the 3 roundings of x itself);
    # a weight is alpha T: relative error gamma_4 + the exponent's error (+ the same on alpha through exp(-x_k), x_k <= sum|x|)
    dn = np.linalg.norm(d.astype(np.float64), axis=-1)[:, None]
    dz = np.concatenate([np.diff(z.astype(np.float64), axis=-1), np.full((B, 1), 1e10)], -1) * dn
    x = dz * raw[..., 3]
    sx = np.cumsum(np.abs(x[:, :-1]), -1)
    sx = np.concatenate([np.zeros((B, 1)), sx], -1)
    T = np.exp(-np.concatenate([np.zeros((B, 1)), np.cumsum(x[:, :-1], -1)], -1))
    rel_T = np.expm1(R.gamma(n + 10) * sx) + R.gamma(4)
    # alpha = 1 - exp(-relu x): absolute error (gamma_3 |x| + u) exp(-relu x) + u
    ax = np.maximum(x, 0)
    err_alpha = (R.gamma(4) * ax + R.U32) * np.exp(-ax) + R.U32
    alpha = 1 - np.exp(-ax)
    bound_w = (err_alpha * T + alpha * T * rel_T) * (1 + 1e-3) + R.U32 * np.abs(o_w) + 1e-45
    assert (np.abs(w.v - o_w) <= bound_w).all()
    # sums over the ray: the weights' own errors plus gamma_(n+1) sum|w c| for the summation and the products
    for got, want, c in ((acc, o_acc[:, 0], np.ones_like(o_w)), (depth, o_depth[:, 0], z.astype(np.float64))):
        bound = (bound_w * np.abs(c)).sum(-1) + R.gamma(n + 8) * np.abs(o_w * c).sum(-1)
        assert (np.abs(got.v - want) <= bound).all()
    for ch in range(3):
        c = raw[..., ch].astype(np.float64)
        bound = (bound_w * np.abs(c)).sum(-1) + R.gamma(n + 8) * np.abs(o_w * c).sum(-1)
        if white:
            bound = bound + bound_w.sum(-1) + R.gamma(n + 8) * np.abs(o_w).sum(-1) + 3 * R.U32 * (1 + np.abs(o_rgb[:, ch]))
        assert (np.abs(rgb.v[:, ch] - o_rgb[:, ch]) <= bound).all()
    # the emulation's own bound is about a device expf only: it must stay a few ulp per weight
    assert (w.e <= (2 * E + 4) * R.ulp(np.maximum(np.abs(w.v), alpha.astype(f32) * 0 + np.abs(w.v))) + (E + 1) * R.ulp(T.astype(f32))).all()
    # disp: NaN exactly where acc == 0, else 1 / max(1e-10, depth / acc)
    assert (np.isnan(disp.v) == (acc.v == 0)).all()


@pytest.mark.parametrize("n", [2, 65, 300])
@pytest.mark.parametrize("white", [False, True])
def test_backward_emulation_against_autograd(n, white):
    """d_raw of the emulation against float64 autograd of the oracle.  The bound is first order in float32 roundoff: the suffix
    sum of n terms G w errs by gamma_(n+12) sum|G w| (+ the weights' relative error, which carries the exponent's
    gamma_(n+10) sum|x|); delta multiplies it."""
    B = 7
    raw, z, d, rng = _inputs(B, n, 31 * n)
    raw[..., 3] = np.clip(raw[..., 3], -0.3, 30)
    g_rgb, g_acc, g_dep = (rng.standard_normal(s).astype(f32) for s in ((B, 3), (B,), (B,)))
    rd = T64(raw).requires_grad_(True)
    rgb, _, acc, _, depth = O.raw2outputs(rd, T64(z), T64(d), 0.0, white)
    ((rgb * T64(g_rgb)).sum() + (acc[:, 0] * T64(g_acc)).sum() + (depth[:, 0] * T64(g_dep)).sum()).backward()
    want = rd.grad.numpy()
    got = R.composite_backward(raw, z, d, g_rgb, g_acc, g_dep, white, E=E)
    dn = np.linalg.norm(d.astype(np.float64), axis=-1)[:, None]
    delta = np.concatenate([np.diff(z.astype(np.float64), axis=-1), np.full((B, 1), 1e10)], -1) * dn
    x = delta * raw[..., 3]
    sx = np.concatenate([np.zeros((B, 1)), np.cumsum(np.abs(x[:, :-1]), -1)], -1)
    w = O.raw2outputs(T64(raw), T64(z), T64(d), 0.0, white)[3][..., 0].numpy()
    T = np.exp(-np.concatenate([np.zeros((B, 1)), np.cumsum(x[:, :-1], -1)], -1))
    gacc = g_acc.astype(np.float64) - (g_rgb.astype(np.float64).sum(-1) if white else 0)
    absG = (np.abs(g_rgb.astype(np.float64))[:, None, :] * np.abs(raw[..., :3])).sum(-1) + np.abs(gacc)[:, None] \
        + np.abs(g_dep.astype(np.float64))[:, None] * z
    if white:
        absG = absG + np.abs(g_rgb.astype(np.float64)).sum(-1)[:, None]
    rel = np.expm1(R.gamma(n + 10) * (sx + np.maximum(x, 0).clip(max=100))) + R.gamma(12)
    term = absG * (np.abs(w) + T * np.exp(-np.maximum(x, 0))) * rel + absG * R.gamma(12) * T
    suffix = np.flip(np.cumsum(np.flip(term, -1), -1), -1) + R.gamma(n + 12) * np.flip(np.cumsum(np.flip(absG * np.abs(w), -1), -1), -1)
    bound_sigma = np.abs(delta) * suffix * 1.01 + R.gamma(2) * np.abs(want[..., 3]) + 1e-30
    assert (np.abs(got.v[..., 3] - want[..., 3]) <= bound_sigma).all()
    bound_rgb = (np.abs(w) * rel + 4 * R.U32 * (np.abs(w) + T))[..., None] * np.abs(g_rgb.astype(np.float64))[:, None, :] + 1e-45
    assert (np.abs(got.v[..., :3] - want[..., :3]) <= bound_rgb).all()


def test_fused_emulation_equals_the_staged_pair():
    B, n = 37, 129
    raw, z, d, rng = _inputs(B, n, 5)
    target = rng.random((B, 3), dtype=f32)
    for white in (False, True):
        for scale in (1.0, 64.0):
            rgb, d_raw, loss, _ = R.composite_mse_backward(raw, z, d, target, white, scale, E)
            f_rgb = R.composite_forward(raw, z, d, white, E=E)[0]
            m_loss, m_grad, _ = R.mse_loss_grad(f_rgb.v, target, scale)
            s_raw = R.composite_backward(raw, z, d, m_grad.reshape(B, 3), None, None, white, E=E)
            assert rgb.v.tobytes() == f_rgb.v.tobytes() and d_raw.v.tobytes() == s_raw.v.tobytes()
            want = float(((f_rgb.v.astype(np.float64) - target) ** 2).mean())
            assert abs(float(loss.v) - want) <= R.gamma(3 * B + 4) * want and abs(float(m_loss) - want) <= R.gamma(3 * B + 4) * want


def test_emulation_is_exact_where_no_expf_is_involved():
    raw, z, d, rng = _inputs(5, 65, 2)
    raw[..., 3] = 0.0
    out = R.composite_forward(raw, z, d, True, E=E)
    assert all(float(o.e.max()) == 0.0 for o in out) and np.isnan(out[1].v).all() and (out[0].v == 1.0).all()
    assert float(R.composite_backward(raw, z, d, np.ones((5, 3), f32), white=True, E=E).e.max()) == 0.0


@pytest.mark.parametrize("lindisp", [False, True])
def test_sampling_emulation_against_oracle(lindisp):
    rng = np.random.default_rng(3)
    B, n = 6, 65
    near = (rng.random(B, dtype=f32) * 3 + 0.5).astype(f32)
    far = (near + rng.random(B, dtype=f32) * 5 + 0.1).astype(f32)
    fn = O.sample_z_lindisp if lindisp else O.sample_z_uniform
    want = fn(torch.from_numpy(near)[:, None], torch.from_numpy(far)[:, None], n).numpy()
    got = R.sample_coarse(near, far, n, lindisp)
    assert got.tobytes() == want.tobytes()              # same float32 operations in the same order
    t = rng.random((B, n), dtype=f32)
    if not lindisp:
        want = O.add_noise_z(torch.from_numpy(got), 0.3, torch.from_numpy(t)).numpy()
        np.testing.assert_array_equal(R.add_noise_z(got, t, 0.3), want)
        np.testing.assert_array_equal(R.sample_coarse(near, far, n, False, 0.3, t), want)


TAGS = ["const", "zero", "peaky", "spike", "jitter", "small", "signed"]


@pytest.mark.parametrize("tag", TAGS)
def test_importance_emulation_on_the_reference_fixture(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "ref_inverse_cdf.npz"))
    z, w, u = (g[f"{tag}_{k}"] for k in "zwu")
    cdf, inds, z_new, z_merged = R.importance(z, w[..., 0], u)
    o_new, o_cdf, o_inds, _, _ = O.inverse_cdf_parts(torch.from_numpy(z), torch.from_numpy(w), torch.from_numpy(u))
    # float64-accumulated CDF rounded per element against torch's float32 cumsum: n additions of values <= 1
    agree = float((inds == o_inds.numpy()).mean())
    if tag != "signed":                                   # (signed weights: pdf values of +-1e4, a CDF far outside [0, 1])
        assert np.abs(cdf - o_cdf.numpy()).max() <= R.gamma(z.shape[1]) * 1.0
        assert agree >= 0.995                             # u within an ulp of a knot may fall on the other side
        np.testing.assert_allclose(z_new, g[f"{tag}_out"], atol=4.0 * 64 * R.gamma(64) + 1e-6)
    assert (np.diff(z_merged, axis=-1) >= 0).all() and z_merged.shape[1] == z.shape[1] + u.shape[1]
    assert np.array_equal(np.sort(np.concatenate([z, z_new], -1), -1), z_merged)
    if tag != "signed":                                   # a monotone CDF: the binary search counts the knots <= u
        assert (inds == (cdf[:, None, :] <= u[:, :, None]).sum(-1)).all()


def test_composite_emulation_on_the_reference_fixture(golden_dir):
    """The emulation on the inputs of the golden raw2outputs fixture against the reference's recorded float32 outputs: both are
    float32 evaluations of the same formula in different orders, so they differ by at most the two forward errors."""
    import json
    g = np.load(os.path.join(golden_dir, "ref_mx_raw2outputs.npz"))
    with open(os.path.join(golden_dir, "ref_mx_meta.json")) as fp:
        std = json.load(fp)["raw2outputs"]["noise_std"]
    tags = sorted(k[:-4] for k in g.files if k.endswith("_raw"))
    assert len(tags) == 9
    for tag in tags:
        raw, z, d = g[f"{tag}_raw"], g[f"{tag}_z"], g[f"{tag}_d"]
        noisy = tag == "noise"
        white = noisy or tag.endswith("_w1")
        out = R.composite_forward(raw, z, d, white, g["noise_noise"] if noisy else None, std if noisy else 0.0, E=E)
        n = z.shape[-1]
        sigma = raw[..., 3] + (g["noise_noise"] * f32(std) if noisy else 0)
        x = np.abs(np.diff(z, axis=-1) * np.linalg.norm(d, axis=-1)[:, None] * sigma[:, :-1]).sum(-1) if n > 1 else np.zeros(len(z))
        for nm, a in zip(("rgb", "disp", "acc", "weights", "depth"), out):
            if nm == "disp":
                continue
            b = g[f"{tag}_{nm}"].reshape(a.v.shape).astype(np.float64)
            amp = np.exp(np.clip(x, 0, 80)).reshape((-1,) + (1,) * (a.v.ndim - 1))        # T can exceed 1 for negative densities
            scale = (np.abs(raw[..., :3]).max() + np.abs(z).max() + 1) * amp
            assert (np.abs(a.v - b) <= 2 * R.gamma(2 * n + 20) * (1 + x.max()) * scale).all(), (tag, nm)


# ---- the merge rule ---------------------------------------------------------------------------------------------------------
def _inf_last_case(seed, n=16, N=32):
    rng = np.random.default_rng(seed)
    z = np.sort(rng.random(n, dtype=f32) * 4 + 2)
    z[-1] = np.inf
    w = rng.random(n, dtype=f32)
    u = rng.random(N, dtype=f32)
    u[-3:] = [0.9999, 0.99995, 0.99999]                  # the last bin: z_mid is inf on both sides, inf - inf
    return z, R.importance(z[None], w[None], u[None])[2][0]


@pytest.mark.parametrize("seed", range(5))
def test_merge_rule_and_the_two_branches(seed):
    """The rule: the exact multiset of coarse and new depths, ascending, ties coarse-first, NaN last.  The ascending branch
    (bitonic network + two rank searches) orders numbers only: taken with a NaN new depth it leaves slots unwritten, which is
    why the kernel sends such a ray to the rank sort."""
    z, z_new = _inf_last_case(seed)
    assert np.isnan(z_new).sum() >= 3
    want = R.merge_rule(z, z_new)
    old, branch = R.merge_transcribed(z, z_new, nan_check=False)
    assert branch == "ascending" and sum(v is None for v in old) > 0          # the defect
    new, branch = R.merge_transcribed(z, z_new)
    assert branch == "general" and None not in new
    assert np.array(new, f32).tobytes() == want.tobytes()
    # finite inputs: both branches obey the rule, ties included
    rng = np.random.default_rng(seed)
    zc = np.sort(np.round(rng.random(24) * 8) / 4).astype(f32)
    zn = (np.round(rng.random(13) * 8) / 4).astype(f32)
    got, branch = R.merge_transcribed(zc, zn)
    assert branch == "ascending" and np.array(got, f32).tobytes() == R.merge_rule(zc, zn).tobytes()
    zs = rng.permutation(zc)
    zs[3] = np.nan
    got, branch = R.merge_transcribed(zs, zn)
    want = R.merge_rule(zs, zn)
    assert branch == "general" and np.array_equal(np.array(got, f32), want, equal_nan=True) and np.isnan(want[-1])


# ---- argument checks --------------------------------------------------------------------------------------------------------
def test_argument_checks_of_the_render_entry_points():
    from nerf_meets_mlx_amd import _native
    lib = _native.lib()
    p = C.c_void_p(16)                                    # never dereferenced: every call below returns before a launch
    OK, E_NULL, E_SHAPE = 0, -1, -2
    for n in (0, 1025, -1):
        assert lib.nerf_composite_forward(p, p, p, 4, n, 0.0, None, 0, p, None, None, None, None, None) == E_SHAPE
        assert lib.nerf_composite_backward(p, p, p, 4, n, 0.0, None, 0, p, None, None, p, None) == E_SHAPE
        assert lib.nerf_composite_mse_backward(p, p, p, 4, n, 0, p, 1.0, None, None, p, None) == E_SHAPE
    assert b"1 <= n <= 1024" in lib.nerf_last_error()
    for n in (1, 0, -3):
        assert lib.nerf_sample_coarse(p, 4, n, 0, 0.0, None, p, None) == E_SHAPE
    assert lib.nerf_add_noise_z(p, p, 4, 0, 1.0, C.c_void_p(32), None) == E_SHAPE
    for n, N in ((1, 8), (257, 8), (64, 0), (64, 513), (256, 513), (257, 511)):
        assert lib.nerf_importance_sample(p, p, p, 4, n, N, 1e-5, None, None, None, None, None) == E_SHAPE, (n, N)
    # NULL with raw_noise_std > 0, perturb > 0 without uniforms, required pointers
    assert lib.nerf_composite_forward(p, p, p, 4, 64, 0.5, None, 0, p, None, None, None, None, None) == E_NULL
    assert lib.nerf_composite_backward(p, p, p, 4, 64, 0.5, None, 0, p, None, None, p, None) == E_NULL
    assert lib.nerf_sample_coarse(p, 4, 64, 0, 0.5, None, p, None) == E_NULL
    assert lib.nerf_composite_forward(p, p, p, 4, 64, 0.0, None, 0, None, None, None, None, None, None) == E_NULL
    assert lib.nerf_composite_backward(p, p, p, 4, 64, 0.0, None, 0, None, None, None, p, None) == E_NULL
    assert lib.nerf_composite_mse_backward(p, p, p, 4, 64, 0, None, 1.0, None, None, p, None) == E_NULL
    assert lib.nerf_importance_sample(None, p, p, 4, 64, 8, 1e-5, None, None, None, None, None) == E_NULL
    assert lib.nerf_mse_loss_grad(None, p, 4, 1.0, None, None, None) == E_NULL
    assert lib.nerf_add_noise_z(p, None, 4, 8, 1.0, C.c_void_p(32), None) == E_NULL
    # in place
    assert lib.nerf_add_noise_z(p, p, 4, 8, 1.0, p, None) == E_SHAPE and b"in-place" in lib.nerf_last_error()
    # count <= 0
    for count in (0, -5):
        assert lib.nerf_mse_loss_grad(p, p, count, 1.0, None, None, None) == E_SHAPE
    # empty launches: nothing is read, NULL pointers included
    assert lib.nerf_sample_coarse(None, 0, 64, 0, 0.0, None, None, None) == OK
    assert lib.nerf_add_noise_z(None, None, 0, 8, 1.0, None, None) == OK
    assert lib.nerf_importance_sample(None, None, None, 0, 64, 8, 1e-5, None, None, None, None, None) == OK
    assert lib.nerf_composite_forward(None, None, None, 0, 64, 0.0, None, 0, None, None, None, None, None, None) == OK
    assert lib.nerf_composite_backward(None, None, None, 0, 64, 0.0, None, 0, None, None, None, None, None) == OK
    assert lib.nerf_composite_mse_backward(None, None, None, 0, 64, 0, None, 1.0, None, None, None, None) == OK
