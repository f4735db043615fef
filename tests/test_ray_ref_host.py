"""The host mirrors of csrc/rays.hip (tests/_ray_ref.py) against something independent, and the power of the bit-exact bar that
tests/test_gpu_rays.py puts on the kernels -- no GPU.

1. Ray generation: directions, origins and pixel coordinates equal the reference-run goldens (tests/golden/ref_get_rays.npz, float64
   directions rounded once to float32) and O.select_coords bit for bit; the unit view directions are within 1 ulp of the float64
   normalisation of the float32 direction.
2. NDC warp: bit-equal to O.ndc_rays evaluated in float32 on the inputs of tests/test_gpu_parity.py::test_ndc_rays, and within that
   test's rtol 2e-5 / atol 2e-6 of the float64 evaluation.
3. Row gather: plain indexing, quiet-NaN rows for indices outside the source.
4. Power.  Each mutation below must leave the bar (bit equality with the mirror) on the inputs of tests/test_gpu_rays.py:
     fx and fy swapped         adversarial camera: every dy differs, so all three rotated components do.  INVISIBLE on the golden
                               cameras (fx == fy there: asserted below), which is why the adversarial camera exists
     cx and cy swapped         adversarial camera; on the goldens only `rect` (W != H) sees it
     rotation transposed       adversarial camera and every golden camera (an orthonormal matrix is not symmetric)
     dx/dz - ox/oz regrouped   as (dx oz - ox dz) / (dz oz): the `random` NDC rays.  It stays inside rtol 2e-5 / atol 2e-6 of the
                               float64 evaluation (asserted below: the older bar lets it through) and differs from the mirror in
                               the last bits of most elements
"""
import os

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import _ray_ref as R

f32, f64 = np.float32, np.float64
GOLDEN_CASES = ("small", "rect", "lego64", "lego800")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _golden(golden_dir, case):
    """(H, W, K, c2w, pixel list, directions [n, 3] float32, origins [n, 3] float32)."""
    g = np.load(os.path.join(golden_dir, "ref_get_rays.npz"))
    H, W = (int(v) for v in g[f"{case}_HW"])
    p = g["lego800_idx"] if case == "lego800" else np.arange(H * W)
    return H, W, g[f"{case}_K"], g[f"{case}_c2w"], p, g[f"{case}_d"].reshape(-1, 3).astype(f32), g[f"{case}_o"].reshape(-1, 3)


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_ray_mirror_equals_the_goldens(golden_dir, case):
    H, W, K, c2w, p, d, o = _golden(golden_dir, case)
    rays, coords = R.ray_gen(p, W, K, c2w, 2.0, 6.0)
    assert rays.shape == (p.size, 11) and rays.dtype == f32 and p.size == (512 if case == "lego800" else H * W)
    assert np.array_equal(_bits(rays[:, 3:6]), _bits(d)) and np.array_equal(_bits(rays[:, 0:3]), _bits(o))
    assert np.array_equal(coords, O.select_coords(torch.from_numpy(np.asarray(p, np.int64)), W).numpy())
    assert (rays[:, 6] == 2.0).all() and (rays[:, 7] == 6.0).all()


def test_origins_of_the_adversarial_camera_are_the_translation():
    H, W, K, c2w = R.adversarial_camera()
    rays, _ = R.ray_gen(np.arange(H * W), W, K, c2w, 0.5, 9.0)
    assert np.array_equal(_bits(rays[:, 0:3]), _bits(np.broadcast_to(c2w[:, 3], (H * W, 3))))
    assert (rays[:, 6] == 0.5).all() and (rays[:, 7] == 9.0).all()


def _view_direction_error(golden_dir):
    """{camera: (relative error, error in ulp of the float32 value)} of the mirror's view directions against the float64
    normalisation of the float32 direction, on the golden cameras and the adversarial one."""
    cams = [(case,) + _golden(golden_dir, case)[1:5] for case in GOLDEN_CASES]
    H, W, K, c2w = R.adversarial_camera()
    cams.append(("adversarial", W, K, c2w, np.arange(H * W)))
    out = {}
    for name, W, K, c2w, p in cams:
        rays, _ = R.ray_gen(p, W, K, c2w, 2.0, 6.0)
        d64 = rays[:, 3:6].astype(f64)
        want = d64 / np.sqrt((d64 * d64).sum(-1, keepdims=True))
        err = np.abs(rays[:, 8:11].astype(f64) - want)
        out[name] = (err / np.abs(want), err / np.spacing(np.abs(want).astype(f32)).astype(f64))
    return out


def test_view_directions_are_one_rounding_from_the_float64_normalisation(golden_dir):
    """float32(d * (1 / sqrt((x x + y y) + z z))) with the arithmetic in float64: the float64 operations leave the product within
    4.5 2^-53 relative of the exact component, so the one rounding to float32 decides: half an ulp, 2^-24 relative.  Both
    bars carry a factor 1 + 2^-24 for the float64 part, which needs 1 + 4.5 2^-29."""
    for name, (rel, ulp) in _view_direction_error(golden_dir).items():
        assert rel.max() <= 2.0 ** -24 * (1 + 2.0 ** -24), (name, rel.max())
        assert ulp.max() <= 0.5 * (1 + 2.0 ** -24), (name, ulp.max())


def test_view_directions_within_one_ulp_of_the_float64_normalisation(golden_dir):
    """Every component within 1 ulp (of the float32 value) of the float64 normalisation of the float32 direction, on the golden
    cameras and the adversarial one.  Float32 arithmetic, d * (1 / sqrtf((x x + y y) + z z)), does NOT meet this: its four
    roundings after the sum of squares allow 4.5 2^-24 relative, and it erred by up to 1.38 / 1.75 / 2.58 / 1.99 / 2.13 ulp
    (small, rect, lego64, lego800, adversarial), which is why write_ray normalises in float64 (asserted below on the mirror of
    the float32 form: the bar has power)."""
    worst = {name: round(float(ulp.max()), 2) for name, (_, ulp) in _view_direction_error(golden_dir).items()}
    print(f"[view directions] worst error in ulp: {worst}")
    assert max(worst.values()) <= 1.0, worst
    H, W, K, c2w, p = _golden(golden_dir, "lego64")[:5]
    d = R.ray_gen(p, W, K, c2w, 2.0, 6.0)[0][:, 3:6]
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    v32 = d * (f32(1.0) / np.sqrt((x * x + y * y) + z * z))[:, None]
    d64 = d.astype(f64)
    want = d64 / np.sqrt((d64 * d64).sum(-1, keepdims=True))
    assert v32.dtype == f32 and (np.abs(v32.astype(f64) - want) / np.spacing(np.abs(want).astype(f32)).astype(f64)).max() > 2.0


def _old_ndc_inputs():
    torch.manual_seed(0)
    o = torch.randn(100, 3); o[:, 2] -= 4.0
    d = torch.randn(100, 3); d[:, 2] = -d[:, 2].abs() - 0.5
    return o, d


def _packed(o, d):
    rays = np.zeros((o.shape[0], 11), f32)
    rays[:, 0:3], rays[:, 3:6] = o.numpy(), d.numpy()
    return rays


def test_ndc_mirror_equals_the_float32_oracle():
    o, d = _old_ndc_inputs()
    got = R.ndc(_packed(o, d), 378, 504, 400.0, 1.0)
    wo, wd = O.ndc_rays(378, 504, 400.0, 1.0, o, d)
    assert wo.dtype == torch.float32
    assert np.array_equal(_bits(got[:, 0:3]), _bits(wo.numpy())) and np.array_equal(_bits(got[:, 3:6]), _bits(wd.numpy()))
    assert not got[:, 6:].any()                                  # columns 6..10 untouched
    wo64, wd64 = O.ndc_rays(378, 504, 400.0, 1.0, o.double(), d.double())
    np.testing.assert_allclose(got[:, 0:3], wo64.numpy(), rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(got[:, 3:6], wd64.numpy(), rtol=2e-5, atol=2e-6)
    # the other input families of the GPU test, where they are finite
    for kind in ("near", "subnormal"):
        rays = R.ndc_inputs(kind, 1000)
        o2, d2 = torch.from_numpy(rays[:, 0:3].copy()), torch.from_numpy(rays[:, 3:6].copy())
        got = R.ndc(rays.copy(), 378, 504, 400.0, 1.0)
        wo, wd = O.ndc_rays(378, 504, 400.0, 1.0, o2, d2)
        assert np.array_equal(_bits(got[:, 0:3]), _bits(wo.numpy())) and np.array_equal(_bits(got[:, 3:6]), _bits(wd.numpy())), kind
        assert np.array_equal(_bits(got[:, 6:]), _bits(rays[:, 6:])), kind
        if kind == "near":                                       # tn == +-0: the origin stays on the near plane, o' z = -1 exactly
            assert (got[:, 2] == -1.0).all()


def test_ndc_inputs_reach_their_edges():
    tiny = R.ndc_inputs("tiny_dz", 1000)
    out = R.ndc(tiny.copy(), 378, 504, 400.0, 1.0)[:, :6]
    assert np.isnan(out).any() and np.isinf(out).any() and np.isfinite(out).any()
    assert (tiny[:, 5] == 0).sum() > 100 and np.abs(tiny[tiny[:, 5] != 0, 5]).min() <= 1.01e-30
    assert np.signbit(tiny[tiny[:, 5] == 0, 5]).any() and not np.signbit(tiny[tiny[:, 5] == 0, 5]).all()


def test_gather_mirror():
    src = np.arange(12, dtype=f32).reshape(4, 3)
    out = R.gather_rows(src, [3, 0, 0, -1, 4, 2 ** 40, 2])
    assert np.array_equal(out[[0, 1, 2, 6]], src[[3, 0, 0, 2]])
    assert (_bits(out[3:6]) == R.QNAN_BITS).all()


# ------------------------------------------------------------------------------------------------ power
def _differs(a, b):
    """Share of elements whose bits differ."""
    return float((_bits(a) != _bits(b)).mean())


def test_swapped_intrinsics_and_a_transposed_rotation_leave_the_bar(golden_dir):
    H, W, K, c2w = R.adversarial_camera()
    p = np.arange(H * W)
    good, _ = R.ray_gen(p, W, K, c2w, 2.0, 6.0)
    Kf, Kc, ct = K.copy(), K.copy(), c2w.copy()
    Kf[0, 0], Kf[1, 1] = K[1, 1], K[0, 0]
    Kc[0, 2], Kc[1, 2] = K[1, 2], K[0, 2]
    ct[:, :3] = c2w[:, :3].T
    for what, args in (("fx <-> fy", (Kf, c2w)), ("cx <-> cy", (Kc, c2w)), ("transposed rotation", (K, ct))):
        bad, _ = R.ray_gen(p, W, *args, 2.0, 6.0)
        share_d, share_v = _differs(bad[:, 3:6], good[:, 3:6]), _differs(bad[:, 8:11], good[:, 8:11])
        print(f"[{what}] adversarial camera: {share_d:.3f} of the directions and {share_v:.3f} of the view directions differ")
        assert share_d > 0.9 and share_v > 0.9, what
    # the golden cameras: fx == fy hides the first swap everywhere, W == H hides the second; the transposed rotation shows on all
    for case in GOLDEN_CASES:
        gH, gW, gK, gc, gp, d, _ = _golden(golden_dir, case)
        swap = gK.copy()
        swap[0, 0], swap[1, 1] = gK[1, 1], gK[0, 0]
        assert _differs(R.ray_gen(gp, gW, swap, gc, 2.0, 6.0)[0], R.ray_gen(gp, gW, gK, gc, 2.0, 6.0)[0]) == 0.0, case
        gt = gc.copy()
        gt[:, :3] = gc[:, :3].T
        assert _differs(R.ray_gen(gp, gW, gK, gt, 2.0, 6.0)[0][:, 3:6], d) > 0.9, case


def test_a_regrouped_ndc_difference_leaves_the_bar_but_not_the_older_one():
    def regrouped(rays, H, W, focal, near):
        focal, near = f32(focal), f32(near)
        sx, sy = -focal / (f32(0.5) * f32(W)), -focal / (f32(0.5) * f32(H))
        ox, oy, oz, dx, dy, dz = (rays[:, k].copy() for k in range(6))
        tn = -(near + oz) / dz
        ox, oy, oz = ox + tn * dx, oy + tn * dy, oz + tn * dz
        return sx * ((dx * oz - ox * dz) / (dz * oz)), sy * ((dy * oz - oy * dz) / (dz * oz))

    for n, rays in ((100, _packed(*_old_ndc_inputs())), (1000, R.ndc_inputs("random", 1000))):
        o64, d64 = torch.from_numpy(rays[:, 0:3].astype(f64)), torch.from_numpy(rays[:, 3:6].astype(f64))
        want = O.ndc_rays(378, 504, 400.0, 1.0, o64, d64)[1].numpy()
        bad = np.stack(regrouped(rays, 378, 504, 400.0, 1.0), -1)
        good = R.ndc(rays.copy(), 378, 504, 400.0, 1.0)[:, 3:5]
        assert bad.dtype == f32
        np.testing.assert_allclose(bad, want[:, :2], rtol=2e-5, atol=2e-6)          # the older bar lets it through
        share = _differs(bad, good)
        print(f"[regrouped NDC difference, {n} rays] {share:.3f} of the elements differ from the mirror")
        assert share > 0.25
