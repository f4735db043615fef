"""Host mirror of the fused positional encodings (a helper module for the tests, not a conftest; csrc/mlp_input.h, the packers of
csrc/mlp_frag.h, csrc/mlp_s16_dev.h and csrc/mlp22.hip, and csrc/encode.hip are the product).

A sine or cosine channel of the view model is  pack(v_sin_f32(t))  where t, in revolutions, is what the kernel's evaluator makes
of the float32 argument a = x f (one float32 multiply: the library is built with -ffp-contract=off) and of the phase ph (0 for a
sine, 1/4 revolution for a cosine).  Everything up to t is float32 arithmetic that a host reproduces BIT FOR BIT:
  SinRevFract    t = fract(f32(f32(a INV_2PI) + ph))                              (bf16 kernels, csrc/mlp.hip)
  SinCodyWaite   k = rint(f32(a INV_2PI));  r = fma(-k, HI, a);  r = fma(-k, LO, r);  t = fma(r, INV_2PI, ph)
                                                                                  (precision 22: csrc/mlp_s16.hip, csrc/mlp22.hip)
The one operation a host cannot reproduce is v_sin_f32 itself; `sin_rev(t)` = sin(2 pi t) in float64 is what a perfect instruction
would return, and the GPU tests allow the instruction an absolute error H around it (tests/test_gpu_encodings.py).
`true_value(a, kind)` is the float64 sine / cosine of the float32 argument: what the encoding is meant to be.

One rounding per fused multiply-add.  `fma32(a, b, c)` computes the product of two float32 numbers in float64, where it is exact
(48 significant bits; no float32 product of interest leaves the float64 exponent range), adds c with the error term of Knuth's
TwoSum, and, where the float64 sum is inexact, moves it to the neighbour with an odd last mantissa bit (round to odd).  Rounding
a round-to-odd 53-bit number to 24 bits to nearest-even equals rounding the exact number once (53 >= 24 + 2).  So the result is
the correctly rounded fused multiply-add for EVERY input, not only where the float64 sum happens to be exact;
tests/test_encoding_host.py checks it against exact rational arithmetic (fractions.Fraction), |k| = 489 included.

v_fract_f32 is x - floor(x) rounded to nearest, with the result clamped to the largest float32 below 1 (0x3f7fffff): for a float32
x the difference is exact in float64 down to |x| = 2^-29, and below that it rounds to 1.0 in either precision, so float64
followed by float32 is the one rounding.

The packers, as values (what the MFMA or the debug reader makes of the packed bits):
  q_bf16         round to nearest even to bf16 (v_cvt_pk_bf16_f32; CvtBf16 and PackBf16 convert the same way)
  q_split_bf16   hi = bf16(v), lo = bf16(v - hi) (the difference is exact), value f32(hi + lo) as nerf_mlp_debug_read adds them
  q_split_f16    hi = fp16(v), lo = fp16((v - hi) 2^11) (exact difference and scaling), value hi + lo 2^-11
"""
import numpy as np

f32 = np.float32
f64 = np.float64

INV_2PI = f32(0.15915494309189535)          # csrc/mlp_input.h
CW_HI = f32(6.2831854820251465)             # 2 pi = HI + LO (SinCodyWaite)
CW_LO = f32(-1.7484556000744487e-07)
HALF_PI_F32 = f32(1.57079637050628662109375)   # csrc/encode.hip (encode_sinusoidal_kernel)
FRACT_MAX = np.array(0x3f7fffff, np.uint32).view(f32)[()]
KIND_ID, KIND_SIN, KIND_COS, KIND_PAD = 0, 1, 2, 3


def freqs(n, freq_mode):
    """fill_freqs of csrc/mlp_input.h: k * k (freq_mode 0, ref_quirks) or 2^k (freq_mode 1), float32."""
    k = np.arange(n)
    return (k * k if freq_mode == 0 else 2 ** k).astype(f32)


def channels(n_freqs, width, dims=3):
    """Columns of a stored encoding: (kind, dim, band) per column -- [x, sin(f0 x), cos(f0 x), sin(f1 x), ...], zero pad behind."""
    out = [(KIND_ID, d, 0) for d in range(dims)]
    for b in range(n_freqs):
        out += [(KIND_SIN, d, b) for d in range(dims)] + [(KIND_COS, d, b) for d in range(dims)]
    return out + [(KIND_PAD, 0, 0)] * (width - len(out))


def argument(x, f):
    """a = x f, one float32 multiply."""
    return (np.asarray(x, f32) * np.asarray(f, f32)).astype(f32)


def true_value(a, kind):
    """float64 sin(a) (kind 1) or sin(a + pi/2) = cos(a) (kind 2) of the float32 argument."""
    a = np.asarray(a, f32).astype(f64)
    return np.where(np.asarray(kind) == KIND_COS, np.cos(a), np.sin(a))


def sin_rev(t):
    """What a perfect v_sin_f32 returns for t revolutions: sin(2 pi t) in float64."""
    return np.sin(2.0 * np.pi * np.asarray(t, f32).astype(f64))


def fma32(a, b, c):
    """float32 fma(a, b, c) with ONE rounding (module docstring)."""
    a, b, c = (np.asarray(v, f32).astype(f64) for v in (a, b, c))
    p = a * b                                                   # exact
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                             # TwoSum: p + c = s + err exactly
    odd = (s.view(np.int64) & 1).astype(bool)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & ~odd, np.nextafter(s, toward), s)
    return s.astype(f32)


def fract32(x):
    """v_fract_f32."""
    x = np.asarray(x, f32).astype(f64)
    return np.minimum((x - np.floor(x)).astype(f32), FRACT_MAX)


def phase_of(kind):
    return np.where(np.asarray(kind) == KIND_COS, f32(0.25), f32(0.0)).astype(f32)


def rev_fract(a, ph):
    """SinRevFract's operand of v_sin_f32."""
    a = np.asarray(a, f32)
    rev = (a * INV_2PI).astype(f32)
    return fract32((rev + np.asarray(ph, f32)).astype(f32))


def cody_waite_k(a):
    return np.rint((np.asarray(a, f32) * INV_2PI).astype(f32)).astype(f32)


def rev_cody_waite(a, ph, lo=CW_LO):
    """SinCodyWaite's operand of v_sin_f32 (lo: the LO constant, for the power check of the host tests)."""
    a = np.asarray(a, f32)
    k = cody_waite_k(a)
    r = fma32(-k, CW_HI, a)
    r = fma32(-k, lo, r)
    return fma32(r, INV_2PI, ph)


# ------------------------------------------------------------------------------------------------ packers
def q_bf16(v):
    """float32 -> bf16, round to nearest even, as a float32 value."""
    u = np.ascontiguousarray(np.asarray(v, f32)).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(f32)


def q_split_bf16(v):
    """split_slots of csrc/mlp_s16_dev.h, decoded like nerf_mlp_debug_read: f32(hi + lo)."""
    v = np.asarray(v, f32)
    hi = q_bf16(v)
    lo = q_bf16((v - hi).astype(f32))
    return (hi + lo).astype(f32)


def q_split_f16(v):
    """split2 of csrc/mlp22.hip as the value the MFMAs see: hi + lo 2^-11 (float64; 22 significant bits)."""
    v = np.asarray(v, f32)
    with np.errstate(over="ignore", under="ignore"):
        hi = v.astype(np.float16)
        r = fma32(hi.astype(f32), f32(-2048.0), (v * f32(2048.0)).astype(f32))
        lo = r.astype(np.float16)
    return hi.astype(f64) + lo.astype(f64) / 2048.0


def half_step(q, s):
    """How far packer q moves a value of size |s| at most (float64): half a step of its values, 2^-bits |s|.  bf16 keeps 8
    significant bits; the split pairs keep hi's bits + lo's bits, and lo's sign is one more: 2^-17 and 2^-22 (lo of the fp16 pair
    loses a bit where v - hi needs 12).  Below the normal range of the format the step stops shrinking: the floor."""
    bits, floor = {q_bf16: (8, 2.0 ** -134), q_split_bf16: (17, 2.0 ** -134), q_split_f16: (22, 2.0 ** -36)}[q]
    return np.maximum(2.0 ** -bits * np.abs(np.asarray(s, f64)), floor)


def ulp32(x):
    """Spacing of float32 at |x| (float64)."""
    x = np.minimum(np.abs(np.asarray(x, f64)), f64(np.finfo(f32).max)).astype(f32)
    return np.spacing(x).astype(f64)


# ------------------------------------------------------------------------------------------------ whole rows
def stored_row_parts(x, n_freqs, width, freq_mode, evaluator):
    """For inputs x [M, 3]: per column of the stored encoding (M x width arrays) the channel kind, the float32 argument a, the
    float64 `true` value, and s = sin_rev(t) of `evaluator` ("fract" | "cody_waite"; None: s = true).  Identity columns carry x in
    `a`, `true` and `s`; pad columns zeros."""
    x = np.asarray(x, f32)
    fr = freqs(n_freqs, freq_mode)
    ch = channels(n_freqs, width)
    kind = np.array([c[0] for c in ch])
    dim = np.array([c[1] for c in ch])
    band = np.array([c[2] for c in ch])
    xs = x[:, dim]
    a = argument(xs, fr[band][None, :])
    wave = (kind == KIND_SIN) | (kind == KIND_COS)
    a = np.where(wave[None, :], a, np.where(kind[None, :] == KIND_ID, xs, f32(0))).astype(f32)
    true = np.where(wave[None, :], true_value(a, kind[None, :]), a.astype(f64))
    if evaluator is None:
        s = true
    else:
        ph = np.broadcast_to(phase_of(kind)[None, :], a.shape)
        t = rev_fract(a, ph) if evaluator == "fract" else rev_cody_waite(a, ph)
        s = np.where(wave[None, :], sin_rev(t), a.astype(f64))
    return np.broadcast_to(kind[None, :], a.shape), a, true, s
