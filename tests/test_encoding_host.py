"""The host mirror of the fused positional encodings (tests/_encoding_ref.py) against exact arithmetic, and what the mirror says
about the Cody-Waite reduction of csrc/mlp_input.h (SinCodyWaite) -- no GPU.

1. fma32 (one rounding per fused multiply-add) equals exact rational arithmetic rounded once, on the three fused steps of the
   reduction at random arguments, at |k| = 489 (|x| = 6 at the top frequency 2^9), and on adversarial triples whose float64 sum is
   inexact.
2. Each packer mirror is monotone non-decreasing and idempotent on more than 10^6 sorted floats ([-6, 6], [-1, 1], |v| <= 1e-4
   down to subnormals).  The interval checks of tests/test_gpu_encodings.py rest on both properties.
3. The reduction error |sin(2 pi t) - sin(a + phase)|, both in float64, over |x| <= 6 and |x| <= 64, both frequency modes and both
   phases, stays under the ANALYTIC sum of its terms (assembled below from the header's constants, not from the measurement).
4. Power: with the sign of LO flipped in the mirror the same samples, already at |x| <= 1 with the 2^k frequencies, exceed ten
   times the largest bar the GPU tests put on v_sin_f32's own error -- a sign error in LO cannot pass tests/test_gpu_encodings.py;
   and a bf16 packer that truncates leaves the interval check of the GPU tests for about half of all values.
"""
from fractions import Fraction

import numpy as np
import pytest

from tests import _encoding_ref as E

f32, f64 = np.float32, np.float64
H_CAP = 7.7e-7                    # the largest H tests/test_gpu_encodings.py may use (its docstring)


def _round_f32(q):
    """A Fraction rounded ONCE to float32, to nearest even (normal range)."""
    if q == 0:
        return f32(0.0)
    sign = -1 if q < 0 else 1
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    e = max(e, -126)
    scaled = q / Fraction(2) ** (e - 23)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return f32(sign * float(n) * 2.0 ** (e - 23))


def _fma_exact(a, b, c):
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_fma_mirror_equals_rational_arithmetic():
    rng = np.random.default_rng(1)
    # arguments whose k is +-489 exactly: a = x f at the top frequency 2^9 with |x| just under 6, and a spread over |x| <= 64
    near = (f32(489.0) * E.CW_HI + rng.uniform(-3.0, 3.0, 500).astype(f32)).astype(f32)
    near = np.concatenate([near, -near])
    assert set(np.unique(np.abs(E.cody_waite_k(near)))) == {489.0}
    x = np.concatenate([rng.uniform(-64, 64, 1800), rng.uniform(-6, 6, 1000), rng.uniform(-1e-3, 1e-3, 200)]).astype(f32)
    fr = np.concatenate([E.freqs(10, 0), E.freqs(10, 1)])
    a = np.concatenate([near, E.argument(x, fr[rng.integers(0, 20, x.size)])])
    ph = np.where(rng.integers(0, 2, a.size) == 1, f32(0.25), f32(0.0)).astype(f32)
    k = E.cody_waite_k(a)
    r1 = E.fma32(-k, E.CW_HI, a)
    r2 = E.fma32(-k, E.CW_LO, r1)
    t = E.fma32(r2, E.INV_2PI, ph)
    bad = 0
    for i in range(a.size):
        bad += _fma_exact(-k[i], E.CW_HI, a[i]) != r1[i]
        bad += _fma_exact(-k[i], E.CW_LO, r1[i]) != r2[i]
        bad += _fma_exact(r2[i], E.INV_2PI, ph[i]) != t[i]
    assert a.size >= 4000 and bad == 0, bad
    # triples whose sum is inexact in float64 (a product of ~2^-40 .. 2^-70 beside an addend that sits on a float32 tie)
    tie = (f32(1.0) + np.arange(1, 400, 2).astype(f64) * 2.0 ** -24)            # halfway between float32 neighbours: not float32
    c = np.concatenate([tie.astype(f32), np.full(200, f32(0.25))])
    pa = rng.uniform(1.0, 2.0, c.size).astype(f32) * f32(2.0) ** rng.integers(-40, -12, c.size).astype(f32)
    pb = rng.uniform(-2.0, 2.0, c.size).astype(f32) * f32(2.0) ** rng.integers(-30, -12, c.size).astype(f32)
    got = E.fma32(pa, pb, c)
    assert all(_fma_exact(pa[i], pb[i], c[i]) == got[i] for i in range(c.size))
    # the tie itself: float64 drops a sliver of 2^-70 and lands ON the float32 tie; one rounding does not
    up, down = f32(1.0 + 2.0 ** -23), f32(1.0 - 2.0 ** -23)
    below = (up, f32(2.0 ** -24) * down, up)            # up + 2^-24 (1 - 2^-46): a sliver BELOW the tie of an odd addend -> stays
    above = (up, f32(2.0 ** -24) * up, f32(1.0))        # 1 + 2^-24 (1 + 2^-22 + 2^-46): above the tie of an even addend -> moves
    assert float(np.float64(up) + np.float64(up) * np.float64(below[1])) == 1.0 + 2.0 ** -23 + 2.0 ** -24, "float64 lands on the tie"
    assert E.fma32(*below) == up == _fma_exact(*below)
    assert E.fma32(*above) == up == _fma_exact(*above)
    assert E.fma32(f32(2.0 ** -24), f32(1.0), f32(1.0)) == f32(1.0) and E.fma32(f32(2.0 ** -24), f32(1.0), up) == f32(1.0 + 2.0 ** -22)


def test_fract_mirror_matches_the_instruction_s_definition():
    x = np.array([0.0, -0.0, 0.25, 1.0, 1.75, -0.25, -1e-10, -1e-30, -2.0 ** -25, 5.9999995, -5.9999995], f32)
    want = [0.0, 0.0, 0.25, 0.0, 0.75, 0.75, float(E.FRACT_MAX), float(E.FRACT_MAX), float(E.FRACT_MAX)]
    got = E.fract32(x)
    assert [float(v) for v in got[:9]] == want
    assert float(E.FRACT_MAX) == 1.0 - 2.0 ** -24 and (got < 1.0).all() and (got >= 0.0).all()
    for v, g in zip(x[9:], got[9:]):
        assert _round_f32(Fraction(float(v)) - Fraction(int(np.floor(v)))) == g


def _sorted_floats():
    rng = np.random.default_rng(2)
    tiny = rng.uniform(-1, 1, 300_000) * 10.0 ** rng.uniform(-45, -4, 300_000)
    v = np.concatenate([rng.uniform(-6, 6, 500_000), rng.uniform(-1, 1, 300_000), tiny, [0.0, -0.0, 1.0, -1.0, 6.0, -6.0]])
    return np.sort(v.astype(f32))


@pytest.mark.parametrize("q,rel", [(E.q_bf16, 2.0 ** -8), (E.q_split_bf16, 2.0 ** -17), (E.q_split_f16, 2.0 ** -22)],
                         ids=["bf16", "split_bf16", "split_f16"])
def test_packer_mirrors_are_monotone_and_idempotent(q, rel):
    v = _sorted_floats()
    assert v.size >= 1_000_000
    out = np.asarray(q(v), f64)
    assert (np.diff(out) >= 0).all(), "not monotone"
    again = np.asarray(q(out.astype(f32)), f64)
    assert np.array_equal(out.astype(f32).astype(f64), out) and np.array_equal(again, out), "not idempotent"
    big = np.abs(v) >= 2.0 ** -14
    assert (np.abs(out - v.astype(f64))[big] <= rel * np.abs(v.astype(f64))[big]).all()
    assert (np.abs(out - v.astype(f64)) <= E.half_step(q, v)).all()


def _samples(limit, mode, n=400_000):
    rng = np.random.default_rng(100 * int(limit) + mode)
    x = rng.uniform(-limit, limit, n).astype(f32)
    fr = E.freqs(10, mode)
    return E.argument(x[:, None], fr[None, :]).reshape(-1)


def _reduction_error(a, ph, lo=E.CW_LO):
    t = E.rev_cody_waite(a, np.full(a.shape, ph, f32), lo)
    want = np.sin(a.astype(f64) + (np.pi / 2 if ph else 0.0))
    return np.abs(E.sin_rev(t) - want), t


def _analytic_bound(kmax):
    """(bound on the reduction error in radians, bound on |r|): the terms of the error of t 2 pi against a + phase."""
    two_pi = Fraction(2 * np.pi)                                  # float64 2 pi; its own error (2.5e-16) is added below
    inv_rel = abs(float(Fraction(float(E.INV_2PI)) * two_pi - 1))                 # relative error of the float32 INV_2PI
    # k = rint(f32(a INV_2PI)) is the nearest integer of a number that is off by half an ulp of k and by k inv_rel: the remainder is
    # at most pi plus that much of a turn
    rmax = np.pi + 2 * np.pi * (float(E.ulp32(kmax)) / 2 + kmax * inv_rel)
    assert rmax < 4.0
    remainders = 2 * 2.0 ** -23                                  # two fused steps, each rounds a remainder below 4 to half an ulp
    revolutions = 2.0 ** -25 * 2 * np.pi                         # t = fma(r, INV_2PI, ph) in [1/2, 1) at most: half an ulp, in radians
    inv = inv_rel * rmax                                         # r INV_2PI 2 pi - r
    split = kmax * (abs(float(two_pi - Fraction(float(E.CW_HI)) - Fraction(float(E.CW_LO)))) + 2.5e-16)    # k (2 pi - HI - LO)
    return remainders + revolutions + inv + split, rmax


@pytest.mark.parametrize("limit", [6, 64])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("ph", [0.0, 0.25])
def test_cody_waite_reduction_error_stays_under_the_analytic_sum(limit, mode, ph):
    a = _samples(limit, mode)
    err, t = _reduction_error(a, f32(ph))
    kmax = float(np.abs(E.cody_waite_k(a)).max())
    bound, rmax = _analytic_bound(kmax)
    print(f"[cody-waite |x|<={limit} mode {mode} phase {ph}] |k| <= {kmax:.0f}, reduction error {err.max():.3e}, bound {bound:.3e}, "
          f"|t| <= {np.abs(t).max():.4f}")
    assert 5.0e-7 < bound < 5.6e-7
    assert np.abs(t).max() <= rmax / (2 * np.pi) + 0.25 + 2.0 ** -24 < 1.0
    assert err.max() <= bound


def test_k_reaches_the_documented_sizes():
    """csrc/mlp_input.h: |k| <= 81 for |x| <= 1 at f = 2^9 (13 at f = 81), 489 at |x| = 6 (77 at f = 81); |k LO| <= 8.6e-5."""
    k = lambda x, f: float(E.cody_waite_k(E.argument(f32(x), f32(f))))
    assert (k(1, 512), k(1, 81), k(6, 512), k(6, 81)) == (81.0, 13.0, 489.0, 77.0)
    assert abs(489 * float(E.CW_LO)) <= 8.6e-5


@pytest.mark.parametrize("mode,limit,factor", [(1, 1, 10), (0, 6, 10), (0, 1, 5)])
def test_a_flipped_lo_exceeds_the_gpu_bar(mode, limit, factor):
    """2^k frequencies: |k| reaches 82 within |x| <= 1 and a flipped LO shows 2.9e-5, more than ten times the bar.  k^2 frequencies
    stop at 81 (|k| <= 13 within |x| <= 1: 4.6e-6, five times the bar) and pass ten times the bar within |x| <= 6; the GPU samples
    cover both ranges in both modes."""
    a = _samples(limit, mode)
    for ph in (0.0, 0.25):
        good, _ = _reduction_error(a, f32(ph))
        flipped, _ = _reduction_error(a, f32(ph), lo=-E.CW_LO)
        print(f"[flipped LO mode {mode} |x|<={limit} phase {ph}] {flipped.max():.3e} against {good.max():.3e}")
        assert good.max() < 5.6e-7
        assert flipped.max() > factor * max(H_CAP, 8.6e-7)


def test_a_truncating_bf16_packer_leaves_the_interval():
    """The interval check Q(s - H) <= stored <= Q(s + H) of the GPU tests against a packer that truncates where it should round
    to nearest: about half of all values land one bf16 step below the interval (the precision-16 bar of the older tests, 3e-2,
    let this through)."""
    a = _samples(6, 1, 20_000)
    s = E.sin_rev(E.rev_fract(a, np.zeros(a.shape, f32)))
    v = s.astype(f32)                                                          # a perfect instruction
    truncated = (v.view(np.uint32) & np.uint32(0xffff0000)).view(f32)
    lo, hi = E.q_bf16((s - H_CAP).astype(f32)), E.q_bf16((s + H_CAP).astype(f32))
    assert ((E.q_bf16(v) >= lo) & (E.q_bf16(v) <= hi)).all()
    outside = (truncated < lo) | (truncated > hi)
    assert outside.mean() > 0.4, outside.mean()
