"""The volume renderer (csrc/sampling.hip, csrc/composite.hip) on the device against the float32 host emulation of
tests/_render_ref.py: depth sampling and the importance sampler bit for bit, compositing within the per-element bound that a device
expf erring by at most E ulp allows (0 wherever no expf is involved).  Every output is sentinel-filled first (tests/_poison.py) and
must be fully written; no output is filtered before it is compared.

E.  The ROCm install this suite was written against ships no table of math-function errors, so E was measured once on an MI355X
through the kernels themselves: with z = [0, 1], |d| = 1 and a large positive last density, weights[1] = 1 * expf(-sigma_0) with every
other operation exact.  Over 2^21 arguments spread over [-103.9, 88.7] (results from the smallest subnormal to FLT_MAX; the tests'
arguments lie inside) the device expf differed from the correctly rounded value by at most 1 ulp, subnormal results included.
E = that maximum + 1 = 2.  `test_expf_error_is_within_E` repeats the measurement on a smaller grid and asserts it, so a math
library that errs more fails there and not as a puzzling compositing failure.

The grid-stride loops iterate in: the B > 32 768 compositing cases (forward, backward, fused), the B > 8192 importance case, the
sampling cases with B n > 2048 * 256 and the MSE counts above 64 * 256.
"""
import numpy as np
import pytest
import torch

from tests import _poison as P
from tests import _render_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = 2.0
f32 = np.float32


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def same_bits(got, want, name):
    """Bit for bit (any NaN matches any NaN: the sentinel is excluded by unwritten() == 0)."""
    assert P.unwritten(got) == 0, name
    g, w = host(got), np.asarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape, g.dtype, w.dtype)
    it = np.int32 if g.itemsize == 4 else np.int64
    bad = g.view(it) != w.view(it)
    if g.dtype.kind == "f":
        bad &= ~(np.isnan(g) & np.isnan(w))
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0]}: " \
                          f"{g[bad][0]!r} != {w[bad][0]!r}"


def within(got, ref, name):
    """Every element: the emulation's bits, or NaN where it has NaN, or inside its bound."""
    assert P.unwritten(got) == 0, name
    g = host(got).reshape(ref.v.shape)
    with np.errstate(all="ignore"):
        err = np.abs(g.astype(np.float64) - ref.v.astype(np.float64))
        ok = (g.view(np.int32) == ref.v.view(np.int32)) | (np.isnan(g) & np.isnan(ref.v)) | (err <= ref.e)
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{name}: {int((~ok).sum())} of {ok.size} outside the bound, first at {i}: got {g[i]!r}, "
                             f"emulation {ref.v[i]!r}, |diff| {err[i]:.3e} > bound {ref.e[i]:.3e}")


def rays_of(d, near=2.0, far=6.0, rng=None):
    B = d.shape[0]
    r = np.zeros((B, 11), f32)
    if rng is not None:
        r[:, 0:3] = rng.standard_normal((B, 3))
    r[:, 3:6] = d
    r[:, 6], r[:, 7] = near, far
    return r


def composite_inputs(B, n, seed, lo=-0.5, hi=50.0):
    """As `_composite_inputs` of test_gpu_parity.py: uneven ascending depths, signed densities (the un-ReLU'd transmittance)."""
    rng = np.random.default_rng(seed)
    z = np.sort(rng.random((B, n), dtype=f32) * 4 + 2, -1)
    raw = rng.standard_normal((B, n, 4)).astype(f32)
    raw[..., 3] = np.clip(raw[..., 3] * 3, lo, hi)
    d = rng.standard_normal((B, 3)).astype(f32)
    return raw, z, d, rng


# ------------------------------------------------------------------------------------------------------------------- expf
def test_expf_error_is_within_E():
    a = np.linspace(-103.9, 88.7, 1 << 16).astype(f32)
    B = a.size
    raw = np.zeros((B, 2, 4), f32)
    raw[:, 0, 3], raw[:, 1, 3] = -a, 1.0                 # x_0 = -a, x_1 = 1e10: alpha_1 = 1, T_1 = expf(a)
    z = np.tile(np.array([0.0, 1.0], f32), (B, 1))
    d = np.tile(np.array([1.0, 0.0, 0.0], f32), (B, 1))
    w = host(P.composite_forward_into(dev(raw), dev(z), dev(rays_of(d)), want=("rgb", "weights"))["weights"])[:, 1]
    want = R.exp32(a)
    ulps = np.abs(w.astype(np.float64) - want.astype(np.float64)) / R.ulp(want)
    print(f"device expf: max {ulps.max():.2f} ulp of the correctly rounded value over [{a[0]}, {a[-1]}] "
          f"(subnormal results: {ulps[want < np.finfo(f32).tiny].max():.2f})")
    assert ulps.max() <= E - 1


# --------------------------------------------------------------------------------------------------------------- sampling
@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("perturb", [0.0, 1.0, 0.3])
@pytest.mark.parametrize("B,n", [(1, 2), (37, 64), (5, 193), (8200, 65)])          # 8200 * 65 > 2048 * 256: two trips
def test_sample_coarse(lindisp, perturb, B, n):
    rng = np.random.default_rng(B * 1000 + n)
    near = (rng.random(B, dtype=f32) * 3 + 0.5).astype(f32)
    far = near + rng.random(B, dtype=f32) * 5
    far[::7] = near[::7]                                 # near == far
    if lindisp:
        near[::5] = 0.0                                  # the literal formula divides by near (1 - t) and far t
    rays = rays_of(np.ones((B, 3), f32), near, far)
    t = rng.random((B, n), dtype=f32)
    assert B * n <= R.ELEMENTWISE_CAP or B == 8200
    got = P.sample_coarse_into(dev(rays), n, lindisp, perturb, dev(t) if perturb > 0 else None)
    same_bits(got, R.sample_coarse(near, far, n, lindisp, perturb, t), "z")


@pytest.mark.parametrize("B,n", [(3, 1), (4, 2), (33, 65), (4100, 128)])           # 4100 * 128 > 2048 * 256
@pytest.mark.parametrize("strength", [1.0, 0.3])
def test_add_noise_z(B, n, strength):
    rng = np.random.default_rng(B + n)
    z = np.sort(rng.random((B, n), dtype=f32) * 4 + 2, -1)
    t = rng.random((B, n), dtype=f32)
    same_bits(P.add_noise_z_into(dev(z), dev(t), strength), R.add_noise_z(z, t, strength), "z")


# ------------------------------------------------------------------------------------------------------- importance sampler
FAMILIES = ("const", "zero", "peaky", "spike", "jitter", "small", "signed", "allzero_pad", "onehot", "tiny", "nan", "inf")


def importance_inputs(B, n, N, seed, asc=True):
    """Ray b takes weight family b mod 12; u holds exact knots, 0, the largest float below 1 and a NaN."""
    rng = np.random.default_rng(seed)
    z = np.tile(np.linspace(2.0, 6.0, n, dtype=f32), (B, 1))
    w = np.zeros((B, n), f32)
    for b in range(B):
        fam = FAMILIES[b % len(FAMILIES)]
        if fam == "const":
            w[b] = 0.02
        elif fam == "peaky":
            w[b] = rng.random(n, dtype=f32) ** 8
        elif fam == "spike":
            w[b, (17 * n) // 64], w[b, (40 * n) // 64] = 1.0, 0.25
        elif fam == "jitter":
            z[b] = np.sort(rng.random(n, dtype=f32) * 4 + 2)
            w[b] = rng.random(n, dtype=f32)
        elif fam == "small":
            z[b] = np.linspace(0.5, 1.5, n, dtype=f32)
            w[b] = rng.random(n, dtype=f32)
        elif fam == "signed":
            w[b] = rng.standard_normal(n).astype(f32) * 0.3
        elif fam == "allzero_pad":
            w[b] = -0.01                                  # w + 0.01 == 0: the sum is below eps, the pad path runs
        elif fam == "onehot":
            w[b, n // 3] = 1.0
        elif fam == "tiny":
            w[b] = -0.01 + 1e-9
        elif fam == "nan":
            w[b] = rng.random(n, dtype=f32)
            w[b, n // 2] = np.nan
        elif fam == "inf":
            w[b] = rng.random(n, dtype=f32)
            w[b, n // 2] = np.inf
    u = rng.random((B, N), dtype=f32)
    cdf = R.importance(z, w, u[:, :1])[0]                # knots of THIS input
    for b in range(B):
        k = min(N, 6)
        u[b, :k] = np.resize(np.concatenate([cdf[b, 1:n:max(1, n // 3)], [0.0, np.nextafter(f32(1), f32(0)), np.nan]]), k)
    return z, w, u.astype(f32)


def check_importance(z, w, u, eps=1e-5):
    got = P.importance_into(dev(z), dev(w), dev(u), eps)
    cdf, inds, z_new, z_merged = R.importance(z, w, u, eps)
    same_bits(got["cdf"], cdf, "cdf")
    same_bits(got["inds"], inds, "inds")
    same_bits(got["z_new"], z_new, "z_new")
    same_bits(got["z_merged"], z_merged, "z_merged")
    return got


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 128, 500, 512])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 128, 129, 191, 192, 193, 256])
def test_importance_shapes(n, N):
    assert n + N <= 768
    check_importance(*importance_inputs(13, n, N, n * 1000 + N))


@pytest.mark.parametrize("B", [1, 3, 4, 5, R.IMPORTANCE_CAP + 5])
def test_importance_ray_counts(B):
    """B above 4 x 2048: every wave reuses its LDS slice on the second trip."""
    z, w, u = importance_inputs(B, 65, 40, B)
    got = check_importance(z, w, u)
    # optional outputs: NULL changes no other output bit
    only = P.importance_into(dev(z), dev(w), dev(u), want=("z_merged",))
    assert P.unwritten(only["z_merged"]) == 0 and P.bits_equal(only["z_merged"], got["z_merged"])
    only = P.importance_into(dev(z), dev(w), dev(u), want=("z_new", "inds"))
    assert P.bits_equal(only["z_new"], got["z_new"]) and torch.equal(only["inds"], got["inds"])


@pytest.mark.parametrize("n,N", [(64, 128), (33, 7), (192, 65), (256, 512)])
@pytest.mark.parametrize("kind", ["ties", "descending", "shuffled_ties", "nan", "inf_last", "neg_inf_first"])
def test_importance_merge_rule(kind, n, N):
    """Coarse depths that drive both merge branches, held to the rule: the exact multiset of coarse and new depths, ascending,
    ties coarse-first, NaN last.  `inf_last` / `neg_inf_first` are ascending lists whose infinite mid points make new depths NaN
    (inf - inf): the ascending branch cannot rank those, such a ray has to take the rank sort."""
    B = 9
    z, w, u = importance_inputs(B, n, N, n + N)
    rng = np.random.default_rng(n * N)
    z = np.sort(rng.random((B, n), dtype=f32) * 4 + 2, -1)
    if kind in ("ties", "shuffled_ties"):
        z = np.round(z * 4) / 4                          # many equal depths, equal mid points: new depths tie with coarse ones
    if kind == "descending":
        z = z[:, ::-1].copy()
    if kind == "shuffled_ties":
        z = rng.permuted(z, axis=1)
    if kind == "nan":
        z[::2, n // 2] = np.nan
    if kind == "inf_last":
        z[:, -1] = np.inf
        u[:, -3:] = [0.9999, 0.99995, 0.99999]           # the last bin
    if kind == "neg_inf_first":
        z[:, 0] = -np.inf
        u[:, -3:] = [1e-5, 2e-5, 3e-5]
    z = z.astype(f32)
    got = check_importance(z, w, u)
    if kind in ("inf_last", "neg_inf_first"):
        assert np.isnan(host(got["z_new"])).any(), "the input was meant to produce NaN new depths"


# --------------------------------------------------------------------------------------------------------- compositing forward
def check_forward(raw, z, d, white, noise=None, std=0.0, name=""):
    rays = rays_of(d, rng=np.random.default_rng(1))
    got = P.composite_forward_into(dev(raw), dev(z), dev(rays), white, dev(noise), std)
    ref = dict(zip(P.FWD_OUTPUTS, R.composite_forward(raw, z, d, white, noise, std, E)))
    for k in P.FWD_OUTPUTS:
        within(got[k], ref[k], f"{name}{k}")
    return got, ref


FWD_N = [1, 2, 63, 64, 65, 128, 129, 192, 193, 255, 256, 257, 300, 511, 512, 513, 700, 1023, 1024]


@pytest.mark.parametrize("white", [0, 1])
@pytest.mark.parametrize("n", FWD_N)
def test_composite_forward(n, white):
    for B in (1, 5, 33):
        raw, z, d, rng = composite_inputs(B, n, 100 * n + B)
        got, ref = check_forward(raw, z, d, white, name=f"B={B} ")
        if B == 33:
            noise = rng.standard_normal((B, n)).astype(f32)
            check_forward(raw, z, d, white, noise, 0.5, name="noise ")
            # optional outputs: NULL changes no bit of the others
            rays = dev(rays_of(d, rng=np.random.default_rng(1)))
            for want in (("rgb",), ("rgb", "weights"), ("rgb", "disp", "depth"), ("rgb", "acc")):
                part = P.composite_forward_into(dev(raw), dev(z), rays, white, want=want)
                for k in want:
                    assert P.unwritten(part[k]) == 0 and P.bits_equal(part[k], got[k]), (want, k)


@pytest.mark.parametrize("white", [1])          # one launch per kernel above the cap: the emulation of 32 775 rays takes seconds
def test_composite_forward_grid_stride(white):
    B = R.COMPOSITE_CAP + 7                              # the second trip of the grid-stride loop
    raw, z, d, _ = composite_inputs(B, 64, 5)
    check_forward(raw, z, d, white)


@pytest.mark.parametrize("n", [1, 64, 65, 300])
@pytest.mark.parametrize("white", [0, 1])
def test_composite_forward_exact_cases(n, white):
    """Where no expf argument is non-zero the bound is 0: the outputs are the emulation's bits.  disp: NaN at acc == 0."""
    B = 6
    raw, z, d, _ = composite_inputs(B, n, n)
    zero = raw.copy()
    zero[..., 3] = 0.0
    got, ref = check_forward(zero, z, d, white, name="sigma=0 ")
    assert all(float(ref[k].e.max()) == 0.0 for k in P.FWD_OUTPUTS)
    assert np.isnan(host(got["disp"])).all() and (host(got["acc"]) == 0).all()
    neg = raw.copy()
    neg[..., 3] = -np.abs(neg[..., 3]) * 0.01             # x <= 0 everywhere: alpha == 0 exactly, T > 1
    got, _ = check_forward(neg, z, d, white, name="sigma<0 ")
    assert np.isnan(host(got["disp"])).all()
    got, ref = check_forward(raw, z, np.zeros_like(d), white, name="|d|=0 ")
    assert float(ref["weights"].e.max()) == 0.0 and (host(got["weights"]) == 0).all()
    big = raw.copy()
    big[..., 3] = 1e6                                     # opaque at the first sample: x_0 >= 4e6 / 300
    even = np.tile(np.linspace(2.0, 6.0, n, dtype=f32), (B, 1))
    got, _ = check_forward(big, even, np.ones_like(d), white, name="opaque ")
    assert (host(got["weights"])[:, 0] == 1.0).all()
    # the 1e-10 floor of disp: depth / acc below it (depths near 0) gives exactly 1e10
    tiny = np.sort(np.abs(z - 2.0) * f32(1e-12), -1).astype(f32)
    got, ref = check_forward(raw, tiny, d, white, name="floor ")
    assert (ref["disp"].v == f32(1.0) / f32(1e-10)).any()


@pytest.mark.parametrize("n", [2, 65, 300])
def test_composite_forward_non_finite_stays_in_its_ray(n):
    B = 8
    raw, z, d, _ = composite_inputs(B, n, 9 * n)
    rays = rays_of(d, rng=np.random.default_rng(1))
    clean = P.composite_forward_into(dev(raw), dev(z), dev(rays), 1)
    for what in ("raw_nan", "raw_inf", "sigma_nan", "sigma_inf", "z_nan", "z_inf", "d_nan", "d_inf"):
        r2, z2, d2 = raw.copy(), z.copy(), d.copy()
        val = np.nan if what.endswith("nan") else np.inf
        k = n // 2
        if what.startswith("raw"):
            r2[5, k, 1] = val
        elif what.startswith("sigma"):
            r2[5, k, 3] = val
        elif what.startswith("z"):
            z2[5, k] = val
        else:
            d2[5, 2] = val
        got, ref = check_forward(r2, z2, d2, 1, name=what + " ")
        for kk in P.FWD_OUTPUTS:
            g, c, e = host(got[kk]), host(clean[kk]), ref[kk].v
            assert (np.isnan(g[5]) == np.isnan(e[5])).all() and (np.isinf(g[5]) == np.isinf(e[5])).all(), (what, kk)
            for b in (4, 6, 7):                           # the other three waves of its workgroup
                assert g[b].tobytes() == c[b].tobytes(), (what, kk, b)


# -------------------------------------------------------------------------------------------------------- compositing backward
BWD_N = [1, 2, 63, 64, 65, 128, 129, 191, 192, 193, 255, 256, 257, 300, 512, 513, 1000, 1024]


def backward_case(B, n, seed, white, d_acc, d_depth, std, x_zero=False):
    raw, z, d, rng = composite_inputs(B, n, seed, lo=-0.3, hi=30.0)
    if x_zero:
        raw[:, ::3, 3] = 0.0                              # x exactly 0: the x > 0 gate is closed there
    g_rgb = rng.standard_normal((B, 3)).astype(f32)
    g_acc = rng.standard_normal(B).astype(f32) if d_acc else None
    g_dep = rng.standard_normal(B).astype(f32) if d_depth else None
    noise = rng.standard_normal((B, n)).astype(f32) if std > 0 else None
    rays = rays_of(d, rng=rng)
    got = P.composite_backward_into(dev(raw), dev(z), dev(rays), dev(g_rgb), dev(g_acc), dev(g_dep), white, dev(noise), std)
    within(got, R.composite_backward(raw, z, d, g_rgb, g_acc, g_dep, white, noise, std, E), "d_raw")
    return got


@pytest.mark.parametrize("white", [0, 1])
@pytest.mark.parametrize("n", BWD_N)
def test_composite_backward(n, white):
    backward_case(33, n, 7 * n, white, True, True, 0.0)
    backward_case(5, n, 7 * n + 1, white, False, False, 0.0, x_zero=True)


@pytest.mark.parametrize("white", [0, 1])
@pytest.mark.parametrize("d_acc,d_depth", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("std", [0.0, 0.7])
@pytest.mark.parametrize("n", [64, 193, 300])
def test_composite_backward_optional_gradients_and_noise(n, std, d_acc, d_depth, white):
    backward_case(9, n, n + 3, white, d_acc, d_depth, std, x_zero=True)


def test_composite_backward_gate_is_strict():
    """sigma == 0 everywhere: x == 0, alpha == 0, T == 1, every bound is 0 and d sigma must be exactly 0 (x > 0 is closed;
    x >= 0 would give delta G)."""
    raw, z, d, rng = composite_inputs(7, 65, 3)
    raw[..., 3] = 0.0
    g = rng.standard_normal((7, 3)).astype(f32)
    ref = R.composite_backward(raw, z, d, g, None, None, True, E=E)
    assert float(ref.e.max()) == 0.0
    got = P.composite_backward_into(dev(raw), dev(z), dev(rays_of(d)), dev(g), white=True)
    same_bits(got, ref.v, "d_raw")
    assert (host(got) == 0).all()


@pytest.mark.parametrize("white", [1])          # one launch per kernel above the cap: the emulation of 32 775 rays takes seconds
def test_composite_backward_grid_stride(white):
    backward_case(R.COMPOSITE_CAP + 7, 64, 11, white, True, False, 0.0)


# ------------------------------------------------------------------------------------------------------- the fused training form
def train_case(B, n, seed, white, grad_scale):
    raw, z, d, rng = composite_inputs(B, n, seed, lo=-0.3, hi=30.0)
    raw[:, ::5, 3] = 0.0
    target = rng.random((B, 3), dtype=f32)
    rays = rays_of(d, rng=rng)
    loss, rgb, d_raw = P.composite_mse_backward_into(dev(raw), dev(z), dev(rays), dev(target), white, grad_scale)
    r_rgb, r_draw, r_loss, mag = R.composite_mse_backward(raw, z, d, target, white, grad_scale, E)
    within(rgb, r_rgb, "rgb")
    within(d_raw, r_draw, "d_raw")
    got_loss = float(host(loss)[0])
    tol = R.gamma(B) * mag + float(r_loss.e)              # the workgroups' terms are added atomically, in any order
    print(f"loss {got_loss!r} emulation {float(r_loss.v)!r} tolerance {tol:.3e}")
    assert abs(got_loss - float(r_loss.v)) <= tol
    # NULL rgb / loss change no other bit
    _, _, d2 = P.composite_mse_backward_into(dev(raw), dev(z), dev(rays), dev(target), white, grad_scale, False, False)
    assert P.unwritten(d2) == 0 and P.bits_equal(d2, d_raw)


@pytest.mark.parametrize("white", [0, 1])
@pytest.mark.parametrize("n", BWD_N)
def test_composite_mse_backward(n, white):
    train_case(33, n, 13 * n, white, 1.0)
    train_case(3, n, 13 * n + 1, white, 128.0)


@pytest.mark.parametrize("white", [1])          # one launch per kernel above the cap: the emulation of 32 775 rays takes seconds
def test_composite_mse_backward_grid_stride(white):
    train_case(R.COMPOSITE_CAP + 7, 64, 17, white, 0.5)


# ----------------------------------------------------------------------------------------------------------------------- MSE
@pytest.mark.parametrize("count", [1, 255, 256, 257, R.MSE_CAP + 300, 3 * R.MSE_CAP + 1])
@pytest.mark.parametrize("grad_scale", [1.0, 3.0])
def test_mse_loss_grad(count, grad_scale):
    rng = np.random.default_rng(count)
    p, t = rng.random(count, dtype=f32), rng.random(count, dtype=f32)
    loss, grad = P.mse_loss_grad_into(dev(p), dev(t), grad_scale)
    r_loss, r_grad, mag = R.mse_loss_grad(p, t, grad_scale)
    same_bits(grad, r_grad, "d_pred")
    assert abs(float(host(loss)[0]) - float(r_loss)) <= R.gamma(count) * mag
    loss2, none = P.mse_loss_grad_into(dev(p), dev(t), grad_scale, want_grad=False)
    assert none is None and abs(float(host(loss2)[0]) - float(r_loss)) <= R.gamma(count) * mag
    none, grad2 = P.mse_loss_grad_into(dev(p), dev(t), grad_scale, want_loss=False)
    assert none is None and P.unwritten(grad2) == 0 and P.bits_equal(grad2, grad)


# --------------------------------------------------------------------------------------------------------------- two streams
def test_forward_and_backward_on_two_streams_match_serial_runs():
    ra, za, da, rng = composite_inputs(4099, 193, 1)
    rb, zb, db, _ = composite_inputs(2051, 300, 2)
    g = rng.standard_normal((2051, 3)).astype(f32)
    A = [dev(ra), dev(za), dev(rays_of(da))]
    Bw = [dev(rb), dev(zb), dev(rays_of(db)), dev(g)]
    fwd = P.composite_forward_into(*A, 1)
    bwd = P.composite_backward_into(*Bw, white=True)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        fwd2 = P.composite_forward_into(*A, 1)
    with torch.cuda.stream(s2):
        bwd2 = P.composite_backward_into(*Bw, white=True)
    torch.cuda.synchronize()
    for k in P.FWD_OUTPUTS:
        assert P.unwritten(fwd2[k]) == 0 and P.bits_equal(fwd2[k], fwd[k]), k
    assert P.unwritten(bwd2) == 0 and P.bits_equal(bwd2, bwd)
