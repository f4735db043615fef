"""The host mirror of csrc/metric.hip (tests/_ssim_ref.py) against the float64 oracle, the condition that makes the derived bound of
tests/test_gpu_ssim.py sharp, and the power of that bound -- no GPU.

1. For every case of `_ssim_ref.CASES` and both windows the means sums / n are within 2e-5 of O.ssim(..., full=True) in float64
   (the project's bar for a float32 evaluation against that oracle).
2. bound < 2^-24 for every case: an error of one float32 ulp in a single output of magnitude >= 0.5 (2^-24 at least) moves the sum
   by more than the bound allows.  This is a condition on the case list (n per image stays under about 12 000), not a measurement.
3. Power.  A mutated mirror must leave the bar |sums - sums_ref| <= bound:
     "tap"   the last window tap dropped at the last valid column of every tile
     "halo"  the staged tile one column short
   Both remove w[ws-1] q from an accumulator that holds the rest of the row, so they are visible exactly where that term is not
   rounded away, i.e. where w[ws-1] is not tiny against the window's centre:
     caught by    images3, byte, signed (w = 5: w[4] / w[2] = 0.018 with the reference's window, 0.41 with the usual one), with
                  both windows; w1 (the only tap: the column reads as zero) with both windows; tiles69 and one_row (w = 11) with
                  the usual window only (w[10] / w[5] = 3.9e-3)
     bit-identical and therefore harmless   w = 11 with the reference's window exp(-(x - c)^2) (w[10] / w[5] = 1.4e-11, below half
                  an ulp of the accumulator) and every w = 33 case (w[32] is 0 in float32 with the reference's window and 1e-25 of
                  the centre with the usual one): no test of the sums can see them, and no result depends on them
   "halo" touches full-width tiles only: one_row (tiles 32 and 1 wide) sees it in its first tile, w1 in three of its four.
"""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import _ssim_ref as S

CAUGHT = {True: ("images3", "byte", "signed", "w1"), False: ("images3", "byte", "signed", "w1", "tiles69", "one_row")}


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("name", sorted(S.CASES))
def test_mirror_matches_the_float64_oracle_and_the_bound_is_sharp(name, quirk):
    c = S.case(name, quirk)
    pred, gt = torch.from_numpy(c["pred"].astype(np.float64)), torch.from_numpy(c["gt"].astype(np.float64))
    want, want_cs = O.ssim(pred, gt, w_size=c["ws"], size_average=False, full=True, ref_quirks=quirk)
    mean = c["sums"] / c["n"]
    err = max(float(np.abs(mean[:, 0] - want.numpy()).max()), float(np.abs(mean[:, 1] - want_cs.numpy()).max()))
    print(f"[ssim mirror {name} quirk={quirk}] n = {c['n']}, mean ssim {mean[:, 0]}, |mirror - float64 oracle| <= {err:.2e}, "
          f"bound <= {c['bound'].max():.2e}")
    assert err < 2e-5
    assert 0.0 < c["bound"].max() < 2.0 ** -24
    assert c["n"] < 12_000
    if c["pred"].shape[0] > 1 and name != "w1":                  # the images' sums differ in the third digit
        assert np.abs(np.diff(mean[:, 0])).min() > 1e-3


def test_constants_follow_the_range_of_pred():
    assert S.constants(S.case("images3", True)["pred"]) == (0.01 ** 2, 0.03 ** 2)
    assert S.constants(S.case("byte", True)["pred"]) == ((0.01 * 255) ** 2, (0.03 * 255) ** 2)
    assert S.constants(S.case("signed", True)["pred"]) == ((0.01 * 2) ** 2, (0.03 * 2) ** 2)


def test_a_single_pixel_plane_has_the_closed_form():
    """w = 1 on 1 x 1 planes: the moments are the pixels, the variances are p p - p p = 0 exactly, cs = c2 / c2 = 1."""
    p, g = np.float32(0.3), np.float32(0.8)
    c1, c2 = np.float32(1e-4), np.float32(9e-4)
    s, cs = S.ssim_pixels(np.full((1, 1), p), np.full((1, 1), g), [1.0], 1e-4, 9e-4)
    assert cs[0, 0] == 1.0
    assert s[0, 0] == ((np.float32(2.0) * (p * g) + c1) * c2) / (((p * p + g * g) + c1) * c2)


@pytest.mark.parametrize("mutate", ["tap", "halo"])
@pytest.mark.parametrize("quirk", [True, False])
def test_a_dropped_tap_and_a_short_halo_leave_the_bar(mutate, quirk):
    for name in sorted(S.CASES):
        c = S.case(name, quirk)
        bad, _ = S.ssim_sums(c["pred"], c["gt"], c["window"], c["c1"], c["c2"], mutate)
        ratio = np.abs(bad - c["sums"]) / c["bound"]
        print(f"[ssim {mutate} {name} quirk={quirk}] |mutated - mirror| / bound: ssim {ratio[:, 0].max():.3g}, cs {ratio[:, 1].max():.3g}")
        if name in CAUGHT[quirk]:
            assert ratio[:, 0].min() > 1.0, (name, ratio)        # every image's ssim sum leaves the bar
        else:
            assert np.array_equal(bad, c["sums"]), (name, ratio)  # bit-identical outputs: nothing to see, nothing lost
