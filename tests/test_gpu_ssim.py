"""csrc/metric.hip nerf_ssim_sums on the GPU against its host mirror (tests/_ssim_ref.py), through the raw entry: the float64 sums
themselves, not the wrapper's float32 mean.

Bar: |sums_dev - sums_ref| <= bound for both columns of every image, where sums_ref is the exact sum (math.fsum) of the mirror's
float32 outputs and bound = n 2^-53 sum |v| is the first-order forward-error bound of a float64 sum of the same n addends in any
order.  The device adds the same addends in an order that depends on tiles, waves and atomics, so nothing is measured into the
bar; tests/test_ssim_ref_host.py shows bound < 2^-24 for every case, i.e. one float32 ulp of one output of magnitude >= 0.5 leaves
it.  Every test prints the observed |sums_dev - sums_ref| / bound.  Measured on an MI355X: 0 in every case -- up to 11 635 float32
addends of magnitude about 1 add without rounding in a float64 accumulator, so the device's sums are the exact ones.

Cases (tests/_ssim_ref.py CASES, each with the reference's window and the usual one): 69 tiles (second trip of the persistent
loop, ragged edge tiles), 66 tiles at w = 33, three different images of two planes (attribution), one full tile and a single
output at w = 33, w = 1, one output row; dynamic ranges 255 and [-1, 1]; 65535 planes; the refusals; a re-used sums buffer.
"""
import numpy as np
import pytest
import torch

from tests import _ssim_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # a copy: the cached cases are read-only


def _run(c, sums=None):
    return S.ssim_sums_into(_dev(c["pred"]), _dev(c["gt"]), c["window"], c["c1"], c["c2"], sums=sums).cpu().numpy()


def _assert_within_bound(got, c, what):
    ratio = np.abs(got - c["sums"]) / c["bound"]
    print(f"\n[ssim {what}] n = {c['n']}, sums {got.tolist()}, |dev - ref| / bound: ssim {ratio[:, 0].max():.3g}, cs {ratio[:, 1].max():.3g}")
    assert got.shape == c["sums"].shape and np.isfinite(got).all(), what
    assert (np.abs(got - c["sums"]) <= c["bound"]).all(), (what, ratio)


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("name", sorted(S.CASES))
def test_sums_equal_the_mirror_within_the_summation_bound(name, quirk):
    c = S.case(name, quirk)
    _assert_within_bound(_run(c), c, f"{name} quirk={quirk}")


def test_wrapper_mean_is_the_rounded_quotient_of_the_sums():
    """ops.metric.SSIM divides the float64 sums in float64 and rounds once: 1 ulp of float32 around float32(sums_ref / n)."""
    from nerf_meets_mlx_amd.ops.metric import SSIM
    c = S.case("tiles69", True)
    got, got_cs = SSIM(True)(_dev(c["pred"]), _dev(c["gt"]), w_size=c["ws"], full=True)
    want = (c["sums"][0] / c["n"]).astype(np.float32)
    for g, w in ((got, want[0]), (got_cs, want[1])):
        assert g.dtype == torch.float32 and abs(float(g) - float(w)) <= float(np.spacing(w)), (float(g), float(w))


@pytest.mark.parametrize("C_", [1, 3])
def test_the_largest_plane_count(C_):
    """N C = 65535 planes of 1 x 1 with w = 1.  C = 1: one addend per image, so each sum IS the closed form of its pixel (0 + v is
    exact).  C = 3: three addends per image, planes 3 i .. 3 i + 2, up to plane 65534."""
    n_img = S.MAX_PLANES // C_
    assert n_img * C_ == S.MAX_PLANES
    rng = np.random.default_rng(5)
    pred = rng.uniform(0, 1, (n_img, C_, 1, 1)).astype(np.float32)
    gt = rng.uniform(0, 1, (n_img, C_, 1, 1)).astype(np.float32)
    c1, c2 = S.constants(pred)
    got = S.ssim_sums_into(_dev(pred), _dev(gt), [1.0], c1, c2).cpu().numpy()
    s, cs = S.ssim_pixels(pred, gt, [1.0], c1, c2)
    if C_ == 1:
        assert np.array_equal(got[:, 0], s.reshape(-1).astype(np.float64)) and np.array_equal(got[:, 1], cs.reshape(-1).astype(np.float64))
        assert (cs == 1.0).all()                                 # p p - p p is exactly 0: cs = c2 / c2
    else:
        want, bound = S.ssim_sums(pred, gt, [1.0], c1, c2)
        ratio = np.abs(got - want) / bound
        print(f"\n[ssim 65535 planes, C = 3] |dev - ref| / bound <= {ratio.max():.3g}")
        assert (np.abs(got - want) <= bound).all()
        assert np.abs(np.diff(want[:, 0])).max() > 0.1           # neighbouring images differ: a shifted attribution shows


def test_refusals_launch_nothing_and_clear_nothing():
    pred = torch.rand(S.MAX_PLANES + 1, 1, 1, 1, device=DEV)
    img = torch.rand(1, 1, 40, 40, device=DEV)
    win34 = [1.0 / 34] * 34
    refused = (
        ("N C = 65536", dict(pred=pred, gt=pred, window=[1.0], n_img=S.MAX_PLANES + 1)),
        ("w = 34", dict(pred=img, gt=img, window=win34, n_img=1)),
        ("H < w", dict(pred=img, gt=img, window=S.window(11, True), n_img=1, shape=(1, 1, 10, 40))),
        ("W < w", dict(pred=img, gt=img, window=S.window(11, True), n_img=1, shape=(1, 1, 40, 10))),
        ("NULL pred", dict(pred=None, gt=img, window=S.window(11, True), n_img=1, shape=(1, 1, 40, 40))),
        ("NULL gt", dict(pred=img, gt=None, window=S.window(11, True), n_img=1, shape=(1, 1, 40, 40))),
        ("NULL window", dict(pred=img, gt=img, window=None, n_img=1, ws=11)),
    )
    for what, kw in refused:
        sums = S.poisoned_sums(kw.pop("n_img"))
        with pytest.raises(ValueError):
            S.ssim_sums_into(kw.pop("pred"), kw.pop("gt"), kw.pop("window"), 1e-4, 9e-4, sums=sums, **kw)
        torch.cuda.synchronize()
        assert S.still_poisoned(sums), what
    with pytest.raises(ValueError):                              # NULL sums
        from nerf_meets_mlx_amd import _native as N
        import ctypes as C
        N.check(N.lib().nerf_ssim_sums(N.ptr(img), N.ptr(img), 1, 1, 40, 40, (C.c_float * 1)(1.0), 1, 1e-4, 9e-4, None, N.stream()))
    # the accepted side of both limits
    ok = S.ssim_sums_into(pred[:S.MAX_PLANES], pred[:S.MAX_PLANES], [1.0], 1e-4, 9e-4)
    assert bool((ok == 1.0).all())                               # identical images: ssim = cs = 1 exactly at w = 1
    assert bool(torch.isfinite(S.ssim_sums_into(img, img, [1.0 / 33] * 33, 1e-4, 9e-4)).all())


def test_a_second_call_clears_the_sums_buffer():
    a, b = S.case("images3", True), S.case("signed", True)
    sums = S.poisoned_sums(3)
    first = _run(a, sums)
    _assert_within_bound(first, a, "first call into the buffer")
    second = _run(b, sums)                                       # the same buffer, now holding the first call's sums
    _assert_within_bound(second, b, "second call into the same buffer")
    assert np.abs(first - second).min() > 1e-3
