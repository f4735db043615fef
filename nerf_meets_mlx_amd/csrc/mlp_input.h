// The input stage of the 8 x 256 view model's forward kernels, once: a sample index becomes a position and a view direction
// (load_sample), those become the 63 + 27 channels of the positional encoding [x, sin(f0 x), cos(f0 x), ...]
// (models/embedding.py:30-71) or are read from an already-embedded row (NeRF.forward(x)), and the channels are placed in the MFMA
// B fragments of the first layer.  Two layouts: channel PAIRS (32x32x16 and the fp32 32x32x2 kernels: element j of lane half h in
// k-step ks is channel kperm(ks, h, j)) and lane GROUPS (16x16x32: element j of lane group g is channel pos_chan16 / dir_chan16).
// An encoder is parameterised by an evaluator of sin(x f + phase) and by a packer (how eight floats become a fragment); the
// packed weight streams (fwd_index, fwd_src16, mlp22.h) assume the same channel maps of mlp_index.h.
// The channel order, the encoders and the row readers use no HIP builtin and no vector type: a host compiler instantiates them
// with an evaluator and a packer of its own (tests/input_layout_check.cpp).
#pragma once
#include "mlp_index.h"
#if defined(__HIPCC__)
#include "common.h"
#define NERF_IN __host__ __device__ __forceinline__
#else
#include <stdint.h>
#define NERF_IN inline
#endif

namespace nerf {

struct PeFreq { float pos[10]; float dir[4]; };
// host: the encoding frequencies of freq_mode 0 (k * k) / 1 (2^k)
static inline void fill_freqs(float* pos, float* dir, int mode) {
  for (int k = 0; k < 10; ++k) pos[k] = mode == 0 ? (float)(k * k) : (float)(1 << k);
  for (int k = 0; k < 4; ++k) dir[k] = mode == 0 ? (float)(k * k) : (float)(1 << k);
}

// channel c of the embedding, c >= limit -> zero pad
struct Chan { int kind, dim, band; };   // kind: 0 identity, 1 sin, 2 cos, 3 zero pad
__host__ __device__ constexpr Chan chan_of(int c, int limit) {
  if (c < 3) return Chan{0, c, 0};
  if (c >= limit) return Chan{3, 0, 0};
  return Chan{((c - 3) % 6) >= 3 ? 2 : 1, (c - 3) % 3, (c - 3) / 6};
}
__host__ __device__ constexpr bool is_wave(const Chan& c) { return c.kind == 1 || c.kind == 2; }
__host__ __device__ constexpr float phase_of(const Chan& c) { return c.kind == 2 ? 0.25f : 0.0f; }      // revolutions: cos(a) = sin(a + 1/4 rev)

// An evaluator EV gives sin(x f + 2 pi ph), ph in {0, 1/4}, as EV::sin_ph(x, f, ph), and the sin | cos of a channel pair as
// EV::pair<KA, KB>(xa, fa, xb, fb, h): lane half 0 holds channel A (kind KA), lane half 1 channel B; only the select is per lane.
struct SinCos { float s, c; };
// evaluators that take the phase as an operand: the lane half selects the operands and ONE evaluation serves both halves
template <class EV>
struct ByPhase {
  template <int KA, int KB>
  static NERF_IN SinCos pair(float xa, float fa, float xb, float fb, int h) {
    const float xv = h ? xb : xa;
    const float fv = h ? fb : fa;
    const float ph = h ? (KB == 2 ? 0.25f : 0.0f) : (KA == 2 ? 0.25f : 0.0f);
    const float s = EV::sin_ph(xv, fv, ph);
    return SinCos{s, s};
  }
};

// ------------------------------------------------------------------------------------------
// channel pairs: register j of k-step KS holds channel C0 = kperm(KS, 0, j) in lane half 0 and C0 + 4 in lane half 1.  Both
// descriptions are compile-time, so the frequency table is never indexed dynamically (no scratch)
// ------------------------------------------------------------------------------------------
template <class EV, int C0, int LIMIT, int NB>
NERF_IN float pair_value(const float (&x)[3], const float (&fr)[NB], int h) {
  constexpr Chan a = chan_of(C0, LIMIT), b = chan_of(C0 + 4, LIMIT);
  const float xa = x[a.dim], xb = x[b.dim];
  SinCos w{0.0f, 0.0f};
  if constexpr (is_wave(a) || is_wave(b)) w = EV::template pair<a.kind, b.kind>(xa, fr[a.band], xb, fr[b.band], h);
  const float va = a.kind == 0 ? xa : a.kind == 1 ? w.s : a.kind == 2 ? w.c : 0.0f;
  const float vb = b.kind == 0 ? xb : b.kind == 1 ? w.s : b.kind == 2 ? w.c : 0.0f;
  return h ? vb : va;
}
template <class EV, int KS, int LIMIT, int NB, int... J>
NERF_IN void pair_values(const float (&x)[3], const float (&fr)[NB], int h, float (&v)[8]) {
  ((v[J] = pair_value<EV, kperm(KS, 0, J), LIMIT, NB>(x, fr, h)), ...);
}
// k-step KS of the encoding of x (LIMIT = 63 channels, NB = 10 bands: position; 27, 4: direction) -> PK::pack(values, out...)
template <class EV, class PK, int KS, int LIMIT, int NB, class... OUT>
NERF_IN void encode_pairs(const float (&x)[3], const float (&fr)[NB], int h, OUT&&... out) {
  float v[8];
  pair_values<EV, KS, LIMIT, NB, 0, 1, 2, 3, 4, 5, 6, 7>(x, fr, h, v);
  PK::pack(v, out...);
}
// the same k-step of an already-embedded row x[m][base + c], c < limit else 0
template <class PK, class... OUT>
NERF_IN void row_pairs(const float* __restrict__ row, int ks, int h, int limit, OUT&&... out) {
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = kperm(ks, h, j);
    v[j] = c < limit ? row[c] : 0.0f;
  }
  PK::pack(v, out...);
}

// ------------------------------------------------------------------------------------------
// lane groups: slot sl = 8 ks + j of lane group g holds channel pos_chan16(ks, g, j) (16 position slots) / dir_chan16(g, j) (8
// direction slots).  The map makes a slot the same (sin | cos, x | y | z) in all four groups wherever it is a sine at all: what
// differs per lane is a frequency and a phase, never the code
// ------------------------------------------------------------------------------------------
__host__ __device__ constexpr Chan group_slot(bool dir, int sl, int g) {
  const int c = dir ? dir_chan16(g, sl) : pos_chan16(sl >> 3, g, sl & 7);
  return c < 0 ? Chan{3, 0, 0} : chan_of(c, dir ? 27 : 63);
}
__host__ __device__ constexpr bool group_slots_uniform() {
  for (int dir = 0; dir < 2; ++dir)
    for (int sl = 0; sl < (dir ? 8 : 16); ++sl)
      for (int g = 1; g < 4; ++g) {
        const Chan a = group_slot(dir, sl, 0), b = group_slot(dir, sl, g);
        if (is_wave(a) != is_wave(b) || (is_wave(a) && a.dim != b.dim)) return false;
      }
  return true;
}
static_assert(group_slots_uniform(), "a slot is a sine of the same coordinate in every lane group, or in none");
// Slots with the same band in every group share one per-lane frequency: freq_twin = the first such slot, freq_reg = the index of
// that frequency among the distinct ones (position: 3 -- bands 2g, 2g + 1, 8 + (g >> 1); direction: 1 -- band g)
__host__ __device__ constexpr int freq_twin(bool dir, int sl) {
  for (int s = 0; s < sl; ++s) {
    bool same = is_wave(group_slot(dir, s, 0));
    for (int g = 0; g < 4; ++g) same = same && group_slot(dir, s, g).band == group_slot(dir, sl, g).band;
    if (same) return s;
  }
  return sl;
}
__host__ __device__ constexpr int freq_reg(bool dir, int sl) {      // (sl = number of slots: the number of distinct frequencies)
  int n = 0;
  for (int s = 0; s < freq_twin(dir, sl) && s < (dir ? 8 : 16); ++s) n += is_wave(group_slot(dir, s, 0)) && freq_twin(dir, s) == s;
  return n;
}
__host__ __device__ constexpr int reg_slot(bool dir, int r) {       // the first slot that uses frequency r
  for (int s = 0; s < (dir ? 8 : 16); ++s) if (is_wave(group_slot(dir, s, 0)) && freq_reg(dir, s) == r) return s;
  return -1;
}
constexpr int POS_FREQS = freq_reg(false, 16), DIR_FREQS = freq_reg(true, 8);
// a slot is a sine or a cosine in all groups, or a sine in the even and a cosine in the odd ones (one per-lane phase serves all of those)
__host__ __device__ constexpr bool group_phases_by_parity() {
  for (int dir = 0; dir < 2; ++dir)
    for (int sl = 0; sl < (dir ? 8 : 16); ++sl) {
      const Chan c0 = group_slot(dir, sl, 0), c1 = group_slot(dir, sl, 1), c2 = group_slot(dir, sl, 2), c3 = group_slot(dir, sl, 3);
      if (!is_wave(c0) || (c0.kind == c1.kind && c0.kind == c2.kind && c0.kind == c3.kind)) continue;
      if (c0.kind != 1 || c1.kind != 2 || c2.kind != 1 || c3.kind != 2) return false;
    }
  return true;
}
static_assert(group_phases_by_parity(), "sin | cos of a slot: the same in all groups, or sin in even and cos in odd groups");

// the per-lane frequencies and the phase for the lane's group (pass-invariant; recomputed per pass, cheaper than keeping them)
struct GroupFreq { float pos[POS_FREQS], dir[DIR_FREQS], ph_odd; int g; };
struct Bands { int of[4]; };                             // the band of frequency r in each group
__host__ __device__ constexpr Bands bands_of(bool dir, int r) {
  const int sl = reg_slot(dir, r);
  return Bands{{group_slot(dir, sl, 0).band, group_slot(dir, sl, 1).band, group_slot(dir, sl, 2).band, group_slot(dir, sl, 3).band}};
}
// (the selects are written out in ONE function, one line per frequency: split into a helper per frequency, hipcc lowers the same
// selects differently and the 48-sample split-fp16 kernel, which sits at the edge of the register file, spills)
NERF_IN GroupFreq group_freqs(const PeFreq& fr, int g) {
  static_assert(POS_FREQS == 3 && DIR_FREQS == 1, "one line per distinct frequency below");
  constexpr Bands a = bands_of(false, 0), b = bands_of(false, 1), c = bands_of(false, 2), d = bands_of(true, 0);
  static_assert(c.of[0] == c.of[1] && c.of[2] == c.of[3], "the third position frequency is shared by two groups");
  GroupFreq q;
  q.pos[0] = g == 0 ? fr.pos[a.of[0]] : g == 1 ? fr.pos[a.of[1]] : g == 2 ? fr.pos[a.of[2]] : fr.pos[a.of[3]];
  q.pos[1] = g == 0 ? fr.pos[b.of[0]] : g == 1 ? fr.pos[b.of[1]] : g == 2 ? fr.pos[b.of[2]] : fr.pos[b.of[3]];
  q.pos[2] = g < 2 ? fr.pos[c.of[0]] : fr.pos[c.of[2]];
  q.ph_odd = (g & 1) ? 0.25f : 0.0f;                    // revolutions: cos(a) = sin(a + 1/4 rev)
  q.dir[0] = g == 0 ? fr.dir[d.of[0]] : g == 1 ? fr.dir[d.of[1]] : g == 2 ? fr.dir[d.of[2]] : fr.dir[d.of[3]];
  q.g = g;
  return q;
}
// slot SL of x (DIR: a view direction, 8 slots = one k-step; else a position, 16 slots = two k-steps) for the lane's group
template <class EV, bool DIR, int SL>
NERF_IN float group_value(const GroupFreq& q, const float (&x)[3]) {
  constexpr Chan c0 = group_slot(DIR, SL, 0), c1 = group_slot(DIR, SL, 1), c2 = group_slot(DIR, SL, 2), c3 = group_slot(DIR, SL, 3);
  if constexpr (is_wave(c0)) {
    constexpr int r = freq_reg(DIR, SL);
    const float f = DIR ? q.dir[r] : q.pos[r];
    return EV::sin_ph(x[c0.dim], f, c0.kind == c1.kind ? phase_of(c0) : q.ph_odd);
  } else if constexpr (c0.kind == 0 && c1.kind == 0 && c2.kind == 0) {      // identity channel g, zero pad in the last group
    static_assert(c3.kind == 3, "three coordinates");
    return q.g == 0 ? x[c0.dim] : q.g == 1 ? x[c1.dim] : q.g == 2 ? x[c2.dim] : 0.0f;
  } else {
    static_assert(c0.kind == 3 && c1.kind == 3 && c2.kind == 3 && c3.kind == 3, "zero pad");
    return 0.0f;
  }
}
template <class EV, bool DIR, int... SL>
NERF_IN void group_values(const GroupFreq& q, const float (&x)[3], float (&v)[DIR ? 1 : 2][8]) {
  ((SL < (DIR ? 8 : 16) ? (void)(v[SL >> 3][SL & 7] = group_value<EV, DIR, DIR ? (SL & 7) : SL>(q, x)) : (void)0), ...);
}
// ... -> PK::pack(values of k-step ks, out[ks]...): every `out` is an array of one fragment per k-step
template <class EV, class PK, bool DIR, class... OUT>
NERF_IN void encode_group(const GroupFreq& q, const float (&x)[3], OUT&... out) {
  float v[DIR ? 1 : 2][8];
  group_values<EV, DIR, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15>(q, x, v);
#pragma unroll
  for (int ks = 0; ks < (DIR ? 1 : 2); ++ks) PK::pack(v[ks], out[ks]...);
}
// the same slots of an already-embedded position (63 channels) or direction (27 channels)
template <class PK, bool DIR, class... OUT>
NERF_IN void row_group(const float* __restrict__ row, int g, OUT&... out) {
  float v[DIR ? 1 : 2][8];
#pragma unroll
  for (int sl = 0; sl < (DIR ? 8 : 16); ++sl) {
    const int ch = DIR ? dir_chan16(g, sl) : pos_chan16(sl >> 3, g, sl & 7);
    v[sl >> 3][sl & 7] = ch >= 0 ? row[ch] : 0.0f;
  }
#pragma unroll
  for (int ks = 0; ks < (DIR ? 1 : 2); ++ks) PK::pack(v[ks], out[ks]...);
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------
// evaluators.  x f is the reference's float32 product in all of them
// ------------------------------------------------------------------------------------------
constexpr float INV_2PI = 0.15915494309189535f;
// bf16 kernels: revolutions, fract, v_sin_f32 (which takes revolutions)
struct SinRevFract : ByPhase<SinRevFract> {
  static __device__ __forceinline__ float sin_ph(float x, float f, float ph) {
    return __builtin_amdgcn_sinf(__builtin_amdgcn_fractf((x * f) * INV_2PI + ph));
  }
};
// split-bf16 training and split-fp16 render: Cody-Waite, a - k 2 pi with 2 pi = HI + LO in two fused steps, then v_sin_f32 on
// revolutions in [-3/4, 3/4].  k = rint(a / 2 pi) grows with the argument a = x f: |k| <= 81 for |x| <= 1 at the top frequency
// f = 2^9 (freq_mode 1; 13 in mode 0, whose top frequency is 81), and |k| <= 489 at |x| = 6, the far end of the scenes' depth
// range (77 in mode 0), where k HI has more bits than a float32 holds.  The steps are fused multiply-adds, so no product is
// rounded, whatever k; each step rounds its sum, a remainder of at most pi in size, once; |k LO| <= 8.6e-5 at |k| = 489.
// Accuracy against the float64 sine of the float32 argument, before the packer: the reduction errs by at most 5.6e-7 (two half
// ulps of a remainder, half an ulp of the revolutions, INV_2PI's rounding; 4.0e-7 seen out to |x| = 64) and v_sin_f32 adds
// 9.3e-8 (measured) -- "float32 tolerance", about five times the error of a float32 sinf, not its last bit
// (tests/test_encoding_host.py, tests/test_gpu_encodings.py).
struct SinCodyWaite : ByPhase<SinCodyWaite> {
  static __device__ __forceinline__ float sin_ph(float x, float f, float ph) {
    const float a = x * f;
    const float k = __builtin_rintf(a * INV_2PI);
    float r = __builtin_fmaf(-k, 6.2831854820251465f, a);
    r = __builtin_fmaf(-k, -1.7484556000744487e-07f, r);
    return __builtin_amdgcn_sinf(__builtin_fmaf(r, INV_2PI, ph));
  }
};
// fp32 kernels: OCML.  One argument reduction (sincosf) where the two lane halves of a register need a sine and a cosine
struct SinOcml {
  static __device__ __forceinline__ float sin_ph(float x, float f, float ph) { return ph != 0.0f ? cosf(x * f) : sinf(x * f); }
  template <int KA, int KB>
  static __device__ __forceinline__ SinCos pair(float xa, float fa, float xb, float fb, int h) {
    const float arg = h ? xb * fb : xa * fa;
    SinCos w{0.0f, 0.0f};
    constexpr bool need_s = KA == 1 || KB == 1, need_c = KA == 2 || KB == 2;
    if (need_s && need_c) sincosf(arg, &w.s, &w.c);
    else if (need_s) w.s = sinf(arg);
    else if (need_c) w.c = cosf(arg);
    return w;
  }
};

// ------------------------------------------------------------------------------------------
// sample loader: sample m of a [B, n] query (M = B n < 2^31, checked on the host: 32-bit divide) -> position o + z d
// (render.py:142; -ffp-contract=off: an unfused multiply and add) and the view direction at ray floats 8..10
// ------------------------------------------------------------------------------------------
// waves and lanes past the end compute on the last sample's inputs and store nothing
__device__ __forceinline__ int64_t clamp_sample(int64_t m, int64_t M) { return m >= M ? M - 1 : m; }
struct Sample { float p[3], d[3]; };
__device__ __forceinline__ Sample load_sample(const float* __restrict__ rays, const float* __restrict__ z, int64_t m, int n) {
  const int64_t ray = (int64_t)((unsigned)m / (unsigned)n);
  const float* rr = rays + ray * NERF_RAY_STRIDE;
  const float zv = z[m];
  Sample s;
#pragma unroll
  for (int c = 0; c < 3; ++c) { s.p[c] = rr[c] + zv * rr[3 + c]; s.d[c] = rr[8 + c]; }
  return s;
}
#endif

}  // namespace nerf
