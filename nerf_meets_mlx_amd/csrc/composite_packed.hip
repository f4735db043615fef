// Compositing of PACKED rays (the output of the occupancy-guided march, include/nerf_hip.h "packed compositing"): ray b owns
// the samples [offsets[b], offsets[b + 1]) of raw [K, 4] / z [K], 0 to 1024 of them.  sigma = trunc_exp(raw[3]), every interval
// is step_world long (no 1e10 on the last one).
//
// HBM-bound: one wavefront per ray, the segment in chunks of 64 samples (one per lane) with the transmittance exponent carried
// from chunk to chunk.  Algorithmic traffic per ray of n samples: forward read 20n + 16 B, write 20 B; training read 2 x 16n
// + 28 B (raw is read again by the reverse pass: L2 hits for a 16 KiB segment), write 16n + 4 B.
#include "common.h"

namespace nerf {
namespace {

constexpr int MAX_CHUNKS = 64;          // the reverse pass keeps chunk c's carried exponent in lane c: segments up to 4096 samples

struct PackedQ {
  float r, g, b, x, alpha, T, w;
};

// the forward quantities of sample k = c0 + lane of a segment ending at s1 (zeros past the end); `carry` = sum of x before c0
__device__ __forceinline__ PackedQ packed_chunk(const float* __restrict__ raw, int64_t c0, int64_t s1, int lane, float step,
                                                float carry, float& chunk_total) {
  PackedQ q;
  const int64_t k = c0 + lane;
  if (k < s1) {
    const float4 rv = *reinterpret_cast<const float4*>(raw + 4 * k);
    q.r = rv.x; q.g = rv.y; q.b = rv.z;
    q.x = expf(rv.w) * step;                                   // trunc_exp forward: exp
    q.alpha = 1.0f - expf(-q.x);
  } else {
    q.r = q.g = q.b = q.x = q.alpha = 0.0f;
  }
  const float incl = wave_scan_incl(q.x, lane);
  const float up = __shfl_up(incl, 1, WAVE);                  // exclusive prefix without incl - x (inf - inf when x = inf)
  const float excl = lane == 0 ? 0.0f : up;
  chunk_total = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, incl), 63));
  q.T = expf(-(carry + excl));
  q.w = q.alpha * q.T;
  return q;
}

// segment of ray b, or (0, 0) with bad = true for offsets outside [0, K] / decreasing / longer than MAX_CHUNKS chunks
__device__ __forceinline__ void segment(const int64_t* __restrict__ offsets, int64_t b, int64_t K, int64_t& s0, int64_t& s1,
                                        bool& bad) {
  s0 = offsets[b];
  s1 = offsets[b + 1];
  bad = !(s0 >= 0 && s0 <= s1 && s1 <= K && s1 - s0 <= (int64_t)MAX_CHUNKS * 64);
  if (bad) s0 = s1 = 0;
}

// ---- the distortion regulariser's per-ray and per-chunk quantities (include/nerf_hip.h "distortion regulariser")
struct DistRay {
  float z0, us;                         // depth of the ray's first sample; |d| / (S step_world)
  bool on;                              // false: |d| zero or not finite, the ray has no distortion term
};

__device__ __forceinline__ DistRay dist_ray(const float* __restrict__ rays, const float* __restrict__ z, int64_t ray, int64_t s0,
                                            int64_t s1, float diag) {
  const float* rr = rays + ray * 11;
  const float dn = (float)sqrt((double)((rr[3] * rr[3] + rr[4] * rr[4]) + rr[5] * rr[5]));      // the march's |d|
  DistRay d;
  d.on = dn > 0.0f && dn <= 3.4028234664e38f;
  d.us = d.on ? dn / diag : 0.0f;
  d.z0 = s0 < s1 ? z[s0] : 0.0f;
  return d;
}

struct DistQ {
  float u, Wl, Ul;                      // position of sample k, sum of w and of w u over the ray's samples before k
};

// the prefixes of sample k = c0 + lane; Wc / Uc = the sums over the chunks before this one, advanced to the next chunk's
__device__ __forceinline__ DistQ dist_chunk(const float* __restrict__ z, int64_t c0, int64_t s1, int lane, const DistRay& d, float w,
                                            float& Wc, float& Uc) {
  DistQ o;
  o.u = c0 + lane < s1 ? (z[c0 + lane] - d.z0) * d.us : 0.0f;
  const float wi = wave_scan_incl(w, lane), ui = wave_scan_incl(w * o.u, lane);
  const float wup = __shfl_up(wi, 1, WAVE), uup = __shfl_up(ui, 1, WAVE);
  o.Wl = Wc + (lane == 0 ? 0.0f : wup);
  o.Ul = Uc + (lane == 0 ? 0.0f : uup);
  Wc += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wi), 63));
  Uc += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ui), 63));
  return o;
}

// ---- One family, two switches.  The forward kernel and the training kernel below each exist in four instantiations over the
// union of the modes' arguments (an instantiation ignores the ones of a switch that is off; the host passes NULL / 0 for them):
//   DIST  the distortion regulariser: L_b of every ray, and in training its adjoint in G_k.  Extra traffic: z (4 B per sample,
//         read again by the reverse pass: L2 hits) and the 12 B of d per ray.
//   BG    a background colour instead of the run-time `white` flag (white or nothing): rgb = sum w c + (1 - acc) * bg.  Forward:
//         bg is one colour for all rays (bg_stride 0) or one per ray (3), read by lane 0.  Training: bg [B, 3] and a straight RGBA
//         target [B, 4] in place of an RGB one.  Extra traffic per ray: 12 B of bg forward; training 16 + 12 B of target + bg
//         instead of 12 B of target.
// With BG off `white` stays a run-time flag and adds (1 - acc) with no multiplication: a background of ones would give the same
// bits but not the same code.
template <bool DIST, bool BG>
__global__ void __launch_bounds__(256) composite_packed_fwd_kernel(const float* __restrict__ raw, const float* __restrict__ z,
                                                                   const int64_t* __restrict__ offsets,
                                                                   const float* __restrict__ rays, int64_t B, int64_t K,
                                                                   float step, float diag, float c1, int white,
                                                                   const float* __restrict__ bg, int bg_stride,
                                                                   float* __restrict__ rgb, float* __restrict__ acc,
                                                                   float* __restrict__ depth, float* __restrict__ dist) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int64_t ray = blockIdx.x * 4 + wv; ray < B; ray += (int64_t)gridDim.x * 4) {
    int64_t s0, s1;
    bool bad;
    segment(offsets, ray, K, s0, s1, bad);
    DistRay dr = {0.0f, 0.0f, false};
    if constexpr (DIST) dr = dist_ray(rays, z, ray, s0, s1, diag);
    float carry = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sa = 0.0f, sd = 0.0f, Wc = 0.0f, Uc = 0.0f, pl = 0.0f, pq = 0.0f;
    for (int64_t c0 = s0; c0 < s1; c0 += 64) {
      float tot;
      const PackedQ q = packed_chunk(raw, c0, s1, lane, step, carry, tot);
      const float zk = c0 + lane < s1 ? z[c0 + lane] : 0.0f;
      sr += q.w * q.r; sg += q.w * q.g; sb += q.w * q.b; sa += q.w; sd += q.w * zk;
      carry += tot;
      if constexpr (DIST) {
        const DistQ e = dist_chunk(z, c0, s1, lane, dr, q.w, Wc, Uc);
        pl += q.w * (e.u * e.Wl - e.Ul); pq += q.w * q.w;
      }
    }
    sr = wave_sum(sr); sg = wave_sum(sg); sb = wave_sum(sb); sa = wave_sum(sa); sd = wave_sum(sd);
    if constexpr (DIST) { pl = wave_sum(pl); pq = wave_sum(pq); }
    if (lane == 0) {
      float L = dr.on ? 2.0f * pl + c1 * pq : 0.0f;
      if constexpr (BG) {
        const float* c = bg + ray * bg_stride;
        sr = sr + (1.0f - sa) * c[0]; sg = sg + (1.0f - sa) * c[1]; sb = sb + (1.0f - sa) * c[2];
      } else if (white) {
        sr = sr + (1.0f - sa); sg = sg + (1.0f - sa); sb = sb + (1.0f - sa);
      }
      if (bad) sr = sg = sb = sa = sd = L = __builtin_nanf("");
      rgb[ray * 3 + 0] = sr; rgb[ray * 3 + 1] = sg; rgb[ray * 3 + 2] = sb;
      if (acc) acc[ray] = sa;
      if (depth) depth[ray] = sd;
      if constexpr (DIST) dist[ray] = L;
    }
  }
}

// Forward (as above) -> rgb -> squared error against the target -> d loss / d raw of every sample of the ray.  The reverse pass
// walks the chunks last to first with the suffix sum of G w carried exactly (no total-minus-prefix), and re-derives each chunk's
// forward quantities from the exponent carried into it, which the forward pass left in lane c of `carries`.
//   dL/dx_k = G_k T_k exp(-x_k) - sum_{k' > k} G_k' w_k',  G_k = gr r_k + gg g_k + gb b_k + gacc
//   d_raw[k] = (w_k gr, w_k gg, w_k gb, dL/dx_k * step * exp(min(raw_k[3], 15)))      (trunc_exp backward)
// DIST: G_k += coef dL_b/dw_k, coef = grad_scale dist_weight / B.  The forward sweep also leaves the chunk-entry sums of w and w u
// in lane c (next to the carried exponent) and ends with the ray's totals W, U; the reverse sweep repeats each chunk's two scans
// (the same operations: the same bits) for Wl_k, Ul_k.
//   dL_b/dw_k = 2 inter_k + (2 delta / 3) w_k,  inter_k = u_k ((2 Wl_k + w_k) - W) - ((2 Ul_k + w_k u_k) - U)
// BG: `target` is RGBA and the target t_c = rgba_c * a + bg_c * (1 - a) is formed here (no composited target through HBM), the
// rendered ray gets (1 - acc) * bg_c, and acc's adjoint becomes
//   gacc = -((gr * bg_r + gg * bg_g) + gb * bg_b)                      (BG off: -(gr + gg + gb) with white, 0 without)
// Two places follow the compiler rather than taste: `bg` is the last argument, and the reverse sweep spells
// the regulariser's work out in two orders, because with either of them changed the <DIST, no BG> form gets another vector
// instruction stream (other registers and another schedule) than the kernel it replaced.
template <bool DIST, bool BG>
__global__ void __launch_bounds__(256) composite_packed_train_kernel(
    const float* __restrict__ raw, const float* __restrict__ z, const int64_t* __restrict__ offsets, const float* __restrict__ rays,
    int64_t B, int64_t K, float step, float diag, float c1, int white, const float* __restrict__ target, float grad_scale, float coef,
    float* __restrict__ loss, float* __restrict__ dist_out, float* __restrict__ rgb_out, float* __restrict__ d_raw,
    const float* __restrict__ bg) {
  __shared__ float part[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float inv = 1.0f / (float)(B * 3), invB = 1.0f / (float)B, c2 = 2.0f * c1;
  float sq = 0.0f, sl = 0.0f;
  for (int64_t ray = blockIdx.x * 4 + wv; ray < B; ray += (int64_t)gridDim.x * 4) {
    int64_t s0, s1;
    bool bad;
    segment(offsets, ray, K, s0, s1, bad);
    DistRay dr = {0.0f, 0.0f, false};
    if constexpr (DIST) dr = dist_ray(rays, z, ray, s0, s1, diag);
    float carry = 0.0f, carries = 0.0f, wcs = 0.0f, ucs = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sa = 0.0f;
    float Wc = 0.0f, Uc = 0.0f, pl = 0.0f, pq = 0.0f;
    int nch = 0;
    for (int64_t c0 = s0; c0 < s1; c0 += 64, ++nch) {
      if (lane == nch) { carries = carry; wcs = Wc; ucs = Uc; }
      float tot;
      const PackedQ q = packed_chunk(raw, c0, s1, lane, step, carry, tot);
      sr += q.w * q.r; sg += q.w * q.g; sb += q.w * q.b; sa += q.w;
      carry += tot;
      if constexpr (DIST) {
        const DistQ e = dist_chunk(z, c0, s1, lane, dr, q.w, Wc, Uc);
        pl += q.w * (e.u * e.Wl - e.Ul); pq += q.w * q.w;
      }
    }
    sr = wave_sum(sr); sg = wave_sum(sg); sb = wave_sum(sb); sa = wave_sum(sa);
    if constexpr (DIST) { pl = wave_sum(pl); pq = wave_sum(pq); }
    float tr, tg, tb, br = 0.0f, bgn = 0.0f, bb = 0.0f;
    if constexpr (BG) {
      const float4 tv = *reinterpret_cast<const float4*>(target + ray * 4);
      br = bg[ray * 3]; bgn = bg[ray * 3 + 1]; bb = bg[ray * 3 + 2];
      tr = tv.x * tv.w + br * (1.0f - tv.w); tg = tv.y * tv.w + bgn * (1.0f - tv.w); tb = tv.z * tv.w + bb * (1.0f - tv.w);
      sr = sr + (1.0f - sa) * br; sg = sg + (1.0f - sa) * bgn; sb = sb + (1.0f - sa) * bb;
    } else {
      tr = target[ray * 3]; tg = target[ray * 3 + 1]; tb = target[ray * 3 + 2];
      if (white) { sr = sr + (1.0f - sa); sg = sg + (1.0f - sa); sb = sb + (1.0f - sa); }
    }
    if (bad) sr = sg = sb = __builtin_nanf("");
    const float er = sr - tr, eg = sg - tg, eb = sb - tb;
    if (lane == 0) {
      sq += er * er; sq += eg * eg; sq += eb * eb;
      if constexpr (DIST) sl += bad ? __builtin_nanf("") : dr.on ? 2.0f * pl + c1 * pq : 0.0f;
      if (rgb_out) { rgb_out[ray * 3] = sr; rgb_out[ray * 3 + 1] = sg; rgb_out[ray * 3 + 2] = sb; }
    }
    const float gr = grad_scale * 2.0f * er * inv, gg = grad_scale * 2.0f * eg * inv, gb = grad_scale * 2.0f * eb * inv;
    const float gacc = 0.0f - (BG ? (gr * br + gg * bgn) + gb * bb : white ? (gr + gg + gb) : 0.0f);
    const float W = Wc, U = Uc;
    float suffix = 0.0f;                                         // sum of G w over the chunks after this one
    for (int c = nch - 1; c >= 0; --c) {
      const int64_t c0 = s0 + (int64_t)c * 64;
      const float cin = __shfl(carries, c, WAVE);
      float Wk = 0.0f, Uk = 0.0f;
      if constexpr (DIST && !BG) { Wk = __shfl(wcs, c, WAVE); Uk = __shfl(ucs, c, WAVE); }       // (the order: see above)
      float tot;
      const PackedQ q = packed_chunk(raw, c0, s1, lane, step, cin, tot);
      float G;
      if constexpr (DIST && !BG) {
        const DistQ e = dist_chunk(z, c0, s1, lane, dr, q.w, Wk, Uk);
        const float inter = e.u * ((2.0f * e.Wl + q.w) - W) - ((2.0f * e.Ul + q.w * e.u) - U);
        G = gr * q.r + gg * q.g + gb * q.b + gacc;
        if (dr.on) G = G + coef * (2.0f * inter + c2 * q.w);
      } else {
        G = gr * q.r + gg * q.g + gb * q.b + gacc;
        if constexpr (DIST) {
          Wk = __shfl(wcs, c, WAVE); Uk = __shfl(ucs, c, WAVE);
          const DistQ e = dist_chunk(z, c0, s1, lane, dr, q.w, Wk, Uk);
          const float inter = e.u * ((2.0f * e.Wl + q.w) - W) - ((2.0f * e.Ul + q.w * e.u) - U);
          if (dr.on) G = G + coef * (2.0f * inter + c2 * q.w);
        }
      }
      const float gw = G * q.w;
      const float rincl = wave_rscan_incl(gw, lane);
      const float dn = __shfl_down(rincl, 1, WAVE);
      const float after = suffix + (lane == 63 ? 0.0f : dn);   // sum over the samples k' > k of the ray
      const int64_t k = c0 + lane;
      if (k < s1) {
        const float sig = raw[4 * k + 3];
        const float dx = G * q.T * expf(-q.x) - after;
        float4 o;
        o.x = q.w * gr; o.y = q.w * gg; o.z = q.w * gb; o.w = dx * step * expf(fminf(sig, 15.0f));
        *reinterpret_cast<float4*>(d_raw + 4 * k) = o;
      }
      suffix += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rincl), 0));
    }
  }
  block_loss_add(part, lane, wv, sq, inv, loss);
  if constexpr (DIST) {
    __syncthreads();                                             // the same 16 B carry the second sum
    block_loss_add(part, lane, wv, sl, invB, dist_out);
  }
}

// ---- round renderer with early ray termination (include/nerf_hip.h "early ray termination").  Per ray: istate int32 [4] = (next
// candidate k, kept count, samples folded, flags), fstate float [6] = (carry, r, g, b, acc, depth).
// init: 40 B of state and 4 B of live id written per ray, nothing read.
__global__ void ert_init_kernel(int64_t B, int* __restrict__ istate, float* __restrict__ fstate, int* __restrict__ live) {
  for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < B; b += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
    for (int q = 0; q < 4; ++q) istate[4 * b + q] = 0;
#pragma unroll
    for (int q = 0; q < 6; ++q) fstate[6 * b + q] = 0.0f;
    live[b] = (int)b;
  }
}

// fold: one lane per live entry, serial over its segment in the header's operation order (so a ray's result does not depend on how
// its samples were split into rounds).  Per entry 4 + 16 + 16 + 24 B read, 40 B written; per sample 20 B read.  The lanes of a wave
// walk segments of different lengths: latency-bound, like the march.
__global__ void ert_fold_kernel(const float* __restrict__ raw, const float* __restrict__ z, const int64_t* __restrict__ offsets,
                                const int* __restrict__ live, int64_t A, int64_t B, int64_t K, float step, float eps,
                                int* __restrict__ istate, float* __restrict__ fstate) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < A; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = live[i];
    if (b < 0 || b >= B) continue;
    int flags = istate[4 * b + 3];
    if (flags & NERF_ERT_TERMINATED) continue;
    const int64_t s0 = offsets[i], s1 = offsets[i + 1];
    float* fs = fstate + 6 * (int64_t)b;
    float carry = fs[0], r = fs[1], g = fs[2], bl = fs[3], acc = fs[4], depth = fs[5];
    int samples = istate[4 * b + 2];
    if (!(s0 >= 0 && s0 <= s1 && s1 <= K)) {                     // bad offsets: the ray's outputs NaN, no access
      carry = r = g = bl = acc = depth = __builtin_nanf("");
      flags |= NERF_ERT_TERMINATED;
    } else {
      for (int64_t k = s0; k < s1; ++k) {
        const float T = expf(-carry);
        if (T < eps) {
          flags |= NERF_ERT_TERMINATED;
          break;
        }
        const float4 rv = *reinterpret_cast<const float4*>(raw + 4 * k);
        const float x = expf(rv.w) * step;
        const float alpha = 1.0f - expf(-x);
        const float w = alpha * T;
        r += w * rv.x; g += w * rv.y; bl += w * rv.z;
        acc += w;
        depth += w * z[k];
        carry += x;
        ++samples;
      }
      // the test of the next sample, made now: the march of the next round then skips the ray (the same outputs, fewer steps)
      if (expf(-carry) < eps) flags |= NERF_ERT_TERMINATED;
    }
    fs[0] = carry; fs[1] = r; fs[2] = g; fs[3] = bl; fs[4] = acc; fs[5] = depth;
    istate[4 * b + 2] = samples;
    istate[4 * b + 3] = flags;
  }
}

// finish: 40 B of state read, 24 B written per ray.  BG: over a background colour (bg, bg_stride as in the packed forward kernel,
// 12 B more read per ray) instead of the `white` flag.
template <bool BG>
__global__ void ert_finish_kernel(const int* __restrict__ istate, const float* __restrict__ fstate, int64_t B, int white,
                                  const float* __restrict__ bg, int bg_stride, float* __restrict__ rgb, float* __restrict__ acc,
                                  float* __restrict__ depth, int* __restrict__ samples) {
  for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < B; b += (int64_t)gridDim.x * blockDim.x) {
    const float* fs = fstate + 6 * b;
    const float a = fs[4];
    if constexpr (BG) {                       // (stores straight from the expressions: through r, g, bl the multiplications swap places)
      const float* c = bg + b * bg_stride;
      rgb[3 * b] = fs[1] + (1.0f - a) * c[0]; rgb[3 * b + 1] = fs[2] + (1.0f - a) * c[1]; rgb[3 * b + 2] = fs[3] + (1.0f - a) * c[2];
    } else {
      float r = fs[1], g = fs[2], bl = fs[3];
      if (white) { r = r + (1.0f - a); g = g + (1.0f - a); bl = bl + (1.0f - a); }
      rgb[3 * b] = r; rgb[3 * b + 1] = g; rgb[3 * b + 2] = bl;
    }
    if (acc) acc[b] = a;
    if (depth) depth[b] = fs[5];
    if (samples) samples[b] = istate[4 * b + 2];
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- host side of the family.  Every entry reports its errors under its own name `who`, in one order: shapes (the sizes, the
// step, then the switches' own settings) before the B == 0 early return, NULL pointers and alignment after it.
template <bool DIST, bool BG>
int packed_shapes(const char* who, int64_t B, int64_t K, float step_world, int march_steps, int bg_stride, float dist_weight) {
  NERF_REQUIRE(B >= 0 && K >= 0, NERF_E_SHAPE, "%s: bad sizes", who);
  NERF_REQUIRE(step_world > 0.0f, NERF_E_SHAPE, "%s: step_world must be > 0", who);
  NERF_REQUIRE(!DIST || (march_steps >= 1 && march_steps <= NERF_MARCH_MAX_STEPS), NERF_E_SHAPE, "%s: need 1 <= march_steps <= %d",
               who, NERF_MARCH_MAX_STEPS);
  NERF_REQUIRE(!BG || bg_stride == 0 || bg_stride == 3, NERF_E_SHAPE, "%s: bg_stride must be 0 (one colour) or 3 (one per ray)", who);
  NERF_REQUIRE(!DIST || (dist_weight >= 0.0f && dist_weight <= 3.4028234664e38f), NERF_E_SHAPE,
               "%s: dist_weight must be finite and >= 0", who);
  return NERF_OK;
}

// one wave per ray, four rays per block, at most 8192 blocks; both kernels begin with the same arguments, among them the
// regulariser's two constants: the box's diagonal S step_world and delta / 3, delta = 1 / S (unused with DIST off, where the
// entries pass march_steps 1)
template <class... P, class... A>
int packed_launch(const char* who, void (*kernel)(P...), void* stream, const float* raw, const float* z, const int64_t* offsets,
                  const float* rays, int64_t B, int64_t K, float step_world, int march_steps, A... rest) {
  const float S = (float)march_steps;
  const dim3 g((unsigned)wave_per_ray_grid(B)), b(256);
  hipLaunchKernelGGL(kernel, g, b, 0, as_stream(stream), raw, z, offsets, rays, B, K, step_world, S * step_world, (1.0f / S) / 3.0f,
                     rest...);
  return check_launch(who);
}

template <bool DIST, bool BG>
int packed_forward(const char* who, const float* raw, const float* z, const int64_t* offsets, const float* rays, int64_t B, int64_t K,
                   float step_world, int march_steps, int white_bkgd, const float* bg, int bg_stride, float* rgb, float* acc,
                   float* depth, float* dist, void* stream) {
  if (const int rc = packed_shapes<DIST, BG>(who, B, K, step_world, march_steps, bg_stride, 0.0f)) return rc;
  if (B == 0) return NERF_OK;
  NERF_REQUIRE(offsets && rgb && (!DIST || (rays && dist)) && (!BG || bg) && (K == 0 || (raw && z)), NERF_E_NULL,
               "%s: NULL pointer", who);
  NERF_REQUIRE(K == 0 || aligned16(raw), NERF_E_SHAPE, "%s: raw must be 16-byte aligned", who);
  return packed_launch(who, composite_packed_fwd_kernel<DIST, BG>, stream, raw, z, offsets, rays, B, K, step_world, march_steps,
                       white_bkgd, bg, bg_stride, rgb, acc, depth, dist);
}

// target: RGB [B, 3], or with BG straight RGBA [B, 4] (one 16-byte load per ray) next to bg [B, 3]
template <bool DIST, bool BG>
int packed_train(const char* who, const float* raw, const float* z, const int64_t* offsets, const float* rays, int64_t B, int64_t K,
                 float step_world, int march_steps, int white_bkgd, const float* target, const float* bg, float grad_scale,
                 float dist_weight, float* loss_out, float* dist_out, float* rgb, float* d_raw, void* stream) {
  if (const int rc = packed_shapes<DIST, BG>(who, B, K, step_world, march_steps, 3, dist_weight)) return rc;
  if (B == 0) return NERF_OK;
  NERF_REQUIRE(offsets && target && (!DIST || rays) && (!BG || bg) && (K == 0 || (raw && d_raw && (!DIST || z))), NERF_E_NULL,
               "%s: NULL pointer", who);
  NERF_REQUIRE((!BG || aligned16(target)) && (K == 0 || (aligned16(raw) && aligned16(d_raw))), NERF_E_SHAPE,
               "%s: %sraw / d_raw must be 16-byte aligned", who, BG ? "target_rgba / " : "");
  return packed_launch(who, composite_packed_train_kernel<DIST, BG>, stream, raw, z, offsets, rays, B, K, step_world, march_steps,
                       white_bkgd, target, grad_scale, grad_scale * dist_weight * (1.0f / (float)B), loss_out, dist_out, rgb, d_raw,
                       bg);
}

template <bool BG>
int ert_finish(const char* who, const int* istate, const float* fstate, int64_t B, int white_bkgd, const float* bg, int bg_stride,
               float* rgb, float* acc, float* depth, int* samples, void* stream) {
  NERF_REQUIRE(B >= 0 && B < (1ll << 31), NERF_E_SHAPE, "%s: need 0 <= B < 2^31", who);
  NERF_REQUIRE(!BG || bg_stride == 0 || bg_stride == 3, NERF_E_SHAPE, "%s: bg_stride must be 0 (one colour) or 3 (one per ray)", who);
  if (B == 0) return NERF_OK;
  NERF_REQUIRE(istate && fstate && rgb && (!BG || bg), NERF_E_NULL, "%s: NULL pointer", who);
  hipLaunchKernelGGL(ert_finish_kernel<BG>, dim3(grid_for(B, 256)), dim3(256), 0, as_stream(stream), istate, fstate, B, white_bkgd, bg,
                     bg_stride, rgb, acc, depth, samples);
  return check_launch(who);
}

}  // namespace
}  // namespace nerf

using namespace nerf;

extern "C" int nerf_composite_packed_forward(const float* raw, const float* z, const int64_t* offsets, int64_t B, int64_t K,
                                             float step_world, int white_bkgd, float* rgb, float* acc, float* depth, void* stream) {
  return packed_forward<false, false>("nerf_composite_packed_forward", raw, z, offsets, nullptr, B, K, step_world, 1, white_bkgd,
                                      nullptr, 0, rgb, acc, depth, nullptr, stream);
}

extern "C" int nerf_composite_packed_distortion(const float* raw, const float* z, const int64_t* offsets, const float* rays,
                                                int64_t B, int64_t K, float step_world, int march_steps, int white_bkgd, float* rgb,
                                                float* acc, float* depth, float* dist, void* stream) {
  return packed_forward<true, false>("nerf_composite_packed_distortion", raw, z, offsets, rays, B, K, step_world, march_steps,
                                     white_bkgd, nullptr, 0, rgb, acc, depth, dist, stream);
}

extern "C" int nerf_composite_packed_forward_bg(const float* raw, const float* z, const int64_t* offsets, int64_t B, int64_t K,
                                                float step_world, const float* bg, int bg_stride, float* rgb, float* acc,
                                                float* depth, void* stream) {
  return packed_forward<false, true>("nerf_composite_packed_forward_bg", raw, z, offsets, nullptr, B, K, step_world, 1, 0, bg,
                                     bg_stride, rgb, acc, depth, nullptr, stream);
}

extern "C" int nerf_composite_packed_distortion_bg(const float* raw, const float* z, const int64_t* offsets, const float* rays,
                                                   int64_t B, int64_t K, float step_world, int march_steps, const float* bg,
                                                   int bg_stride, float* rgb, float* acc, float* depth, float* dist, void* stream) {
  return packed_forward<true, true>("nerf_composite_packed_distortion_bg", raw, z, offsets, rays, B, K, step_world, march_steps, 0,
                                    bg, bg_stride, rgb, acc, depth, dist, stream);
}

extern "C" int nerf_composite_packed_mse_backward(const float* raw, const int64_t* offsets, int64_t B, int64_t K, float step_world,
                                                  int white_bkgd, const float* target, float grad_scale, float* loss_out,
                                                  float* rgb, float* d_raw, void* stream) {
  return packed_train<false, false>("nerf_composite_packed_mse_backward", raw, nullptr, offsets, nullptr, B, K, step_world, 1,
                                    white_bkgd, target, nullptr, grad_scale, 0.0f, loss_out, nullptr, rgb, d_raw, stream);
}

extern "C" int nerf_composite_packed_mse_dist_backward(const float* raw, const float* z, const int64_t* offsets, const float* rays,
                                                       int64_t B, int64_t K, float step_world, int march_steps, int white_bkgd,
                                                       const float* target, float grad_scale, float dist_weight, float* loss_out,
                                                       float* dist_out, float* rgb, float* d_raw, void* stream) {
  return packed_train<true, false>("nerf_composite_packed_mse_dist_backward", raw, z, offsets, rays, B, K, step_world, march_steps,
                                   white_bkgd, target, nullptr, grad_scale, dist_weight, loss_out, dist_out, rgb, d_raw, stream);
}

extern "C" int nerf_composite_packed_mse_backward_bg(const float* raw, const int64_t* offsets, int64_t B, int64_t K, float step_world,
                                                     const float* target_rgba, const float* bg, float grad_scale, float* loss_out,
                                                     float* rgb, float* d_raw, void* stream) {
  return packed_train<false, true>("nerf_composite_packed_mse_backward_bg", raw, nullptr, offsets, nullptr, B, K, step_world, 1, 0,
                                   target_rgba, bg, grad_scale, 0.0f, loss_out, nullptr, rgb, d_raw, stream);
}

extern "C" int nerf_composite_packed_mse_dist_backward_bg(const float* raw, const float* z, const int64_t* offsets, const float* rays,
                                                          int64_t B, int64_t K, float step_world, int march_steps,
                                                          const float* target_rgba, const float* bg, float grad_scale,
                                                          float dist_weight, float* loss_out, float* dist_out, float* rgb,
                                                          float* d_raw, void* stream) {
  return packed_train<true, true>("nerf_composite_packed_mse_dist_backward_bg", raw, z, offsets, rays, B, K, step_world, march_steps,
                                  0, target_rgba, bg, grad_scale, dist_weight, loss_out, dist_out, rgb, d_raw, stream);
}

extern "C" int nerf_ert_init(int64_t B, int* istate, float* fstate, int* live, void* stream) {
  NERF_REQUIRE(B >= 0 && B < (1ll << 31), NERF_E_SHAPE, "nerf_ert_init: need 0 <= B < 2^31");
  if (B == 0) return NERF_OK;
  NERF_REQUIRE(istate && fstate && live, NERF_E_NULL, "nerf_ert_init: NULL pointer");
  hipLaunchKernelGGL(ert_init_kernel, dim3(grid_for(B, 256)), dim3(256), 0, as_stream(stream), B, istate, fstate, live);
  return check_launch("nerf_ert_init");
}

extern "C" int nerf_ert_fold(const float* raw, const float* z, const int64_t* offsets, const int* live, int64_t A, int64_t B,
                             int64_t K, float step_world, float min_transmittance, int* istate, float* fstate, void* stream) {
  NERF_REQUIRE(B >= 0 && B < (1ll << 31) && A >= 0 && A <= B && K >= 0, NERF_E_SHAPE, "nerf_ert_fold: bad sizes");
  NERF_REQUIRE(step_world > 0.0f, NERF_E_SHAPE, "nerf_ert_fold: step_world must be > 0");
  NERF_REQUIRE(min_transmittance >= 0.0f && min_transmittance < 1.0f, NERF_E_SHAPE, "nerf_ert_fold: need 0 <= min_transmittance < 1");
  if (A == 0) return NERF_OK;
  NERF_REQUIRE(offsets && live && istate && fstate && (K == 0 || (raw && z)), NERF_E_NULL, "nerf_ert_fold: NULL pointer");
  NERF_REQUIRE(K == 0 || aligned16(raw), NERF_E_SHAPE, "nerf_ert_fold: raw must be 16-byte aligned");
  hipLaunchKernelGGL(ert_fold_kernel, dim3(grid_for(A, 256)), dim3(256), 0, as_stream(stream), raw, z, offsets, live, A, B, K,
                     step_world, min_transmittance, istate, fstate);
  return check_launch("nerf_ert_fold");
}

extern "C" int nerf_ert_finish(const int* istate, const float* fstate, int64_t B, int white_bkgd, float* rgb, float* acc,
                               float* depth, int* samples, void* stream) {
  return ert_finish<false>("nerf_ert_finish", istate, fstate, B, white_bkgd, nullptr, 0, rgb, acc, depth, samples, stream);
}

extern "C" int nerf_ert_finish_bg(const int* istate, const float* fstate, int64_t B, const float* bg, int bg_stride, float* rgb,
                                  float* acc, float* depth, int* samples, void* stream) {
  return ert_finish<true>("nerf_ert_finish_bg", istate, fstate, B, 0, bg, bg_stride, rgb, acc, depth, samples, stream);
}
