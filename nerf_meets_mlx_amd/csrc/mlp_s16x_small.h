// Device code of the split-bf16 2 x 64 forward (mlp_s16x.hip) that two translation units share: mlp_s16x.hip launches the
// kernels without level weights, mlp_s16x_lw.hip the ones of nerf_ngp_query_fused_lw (LW = true).  Why two units:
// tests/test_isa_inflight_regs.py reads build/mlp_s16x_m0_scan.txt and expects exactly the ten kernels mlp_s16x.hip had before
// the level weights, so the two LW kernels cannot be instantiated there.  Their own scan, build/mlp_s16x_lw_m0_scan.txt
// (check_m0.py --no-scratch, csrc/Makefile), is read by no test: a finding in it fails the build, and that is its only guard.
#pragma once
#include "mlp_s16_dev.h"
#include "mlp_arch2.h"
#include "hash_common.h"
#include "mlp_s16x.h"

namespace nerf {
namespace s16x {

using s16::HL; using s16::split2; using s16::split_slots; using s16::mfma32; using s16::PairSink; using s16::NoPairSink;

template <bool STORE> struct SinkOf { typedef NoPairSink type; };
template <> struct SinkOf<true> { typedef PairSink type; };
template <bool STORE>
__device__ __forceinline__ typename SinkOf<STORE>::type make_sink(void* base, int64_t tile, int64_t stride16, int slot0, int lo_off, int r, int h);
template <>
__device__ __forceinline__ PairSink make_sink<true>(void* base, int64_t tile, int64_t stride16, int slot0, int lo_off, int r, int h) {
  return PairSink{base, tile, stride16, slot0, lo_off, r, h};
}
template <>
__device__ __forceinline__ NoPairSink make_sink<false>(void*, int64_t, int64_t, int, int, int, int) { return NoPairSink{}; }

constexpr int SM_STREAM_BYTES = 64 * 1024;               // 64 fragments of 1 KiB: (hi, lo) pairs of one direction's stream
constexpr int SM_LDS_BYTES = SM_STREAM_BYTES + LN::BI_TOTAL * 4;
// weight source: the whole pair stream resident in LDS (copied once per workgroup); biases behind it
struct LdsPairW {
  __device__ __forceinline__ bf16x8 frag(int f, int lane) { return *reinterpret_cast<const bf16x8*>(ring_smem + f * 1024 + lane * 16); }
  __device__ __forceinline__ void note_stores(int) {}
  __device__ __forceinline__ float4 bias4(int slot) { return *reinterpret_cast<const float4*>(ring_smem + SM_STREAM_BYTES + slot * 4); }
};
__device__ __forceinline__ void lds_load_pairs(const bf16x8* __restrict__ w, const float* __restrict__ bias) {
  for (int i = threadIdx.x; i < 64 * 64; i += blockDim.x) *reinterpret_cast<bf16x8*>(ring_smem + i * 16) = w[i];
  if (bias)
    for (int i = threadIdx.x; i < LN::BI_TOTAL; i += blockDim.x) *reinterpret_cast<float*>(ring_smem + SM_STREAM_BYTES + 4 * i) = bias[i];
  __syncthreads();
}

struct SmallArgs {
  const bf16x8* wf; const bf16x8* wb; const float* bias;
  const float* x;        // [M,48]: 32 position features | 16 direction features
  const float* d_raw;    // [M,4]
  int64_t M;
  float* out;            // [M,4] raw
  float* d_x;            // [M,32] dL/d(position features) or nullptr
  void* acts; void* dz;
  int64_t astride, zstride;
  const float* rays; const float* z; int n; const float* tables; uint32_t T; ResTab rt; float pos_scale, pos_offset;
  int ray_major; int64_t B;
  LevelTab lw;           // per-level weights of nerf_ngp_query_fused_lw: read by the LW kernels only (last member)
};

// B fragments of one sample straight from the float32 hash tables and the view direction (lane / channel mapping of
// mlp.hip:ngp_row_frags): lane (r, h) owns channels kperm(ks, h, j) of k-step ks = levels 8 ks + 4 (j >> 2) + 2 h + ((j & 3) >> 1),
// feature j & 1; SH degree 3 = 16 channels = one k-step.  Interpolated values stay float32 until they are split.
// LW: v = w[l] * interpolation in float32, ahead of the split; w[l] == 0: the lane's gathers of that level are predicated off
// (h selects the levels, so the predicate differs within a wave) and v is +0.
template <bool LW>
__device__ __forceinline__ void ngp_row_pairs(const SmallArgs& a, int64_t m, int h, bf16x8 (&xh)[2], bf16x8 (&xl)[2],
                                              bf16x8 (&dh)[1], bf16x8 (&dl)[1]) {
  const float* rr = a.rays + (int64_t)((uint64_t)m / (unsigned)a.n) * NERF_RAY_STRIDE;
  const float zv = a.z[m];
  // render.py:142, then the scene box -> unit cube map (same two roundings as hash_common.h:point_of)
  const float px = (rr[0] + zv * rr[3]) * a.pos_scale + a.pos_offset, py = (rr[1] + zv * rr[4]) * a.pos_scale + a.pos_offset;
  const float pz = (rr[2] + zv * rr[5]) * a.pos_scale + a.pos_offset;
  const uint32_t mask = a.T - 1;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int l = 8 * ks + 4 * q + 2 * h + e;
        const Corners c = corners_of(px, py, pz, a.rt.res[l], mask);
        if (LW) {
          const float w = h ? a.lw.w[8 * ks + 4 * q + 2 + e] : a.lw.w[8 * ks + 4 * q + e];       // two scalars and a select
          const FeatVec<2> fv = hash_level_lw<false>(a.tables + (size_t)l * a.T * 2, nullptr, c, w);
          v[4 * q + 2 * e] = fv.v[0];
          v[4 * q + 2 * e + 1] = fv.v[1];
        } else {
          const FeatVec<2> fv = hash_level<2>(a.tables + (size_t)l * a.T * 2, c);
          v[4 * q + 2 * e] = fv.v[0];
          v[4 * q + 2 * e + 1] = fv.v[1];
        }
      }
    split_slots<8>(v, &xh[ks], &xl[ks]);
  }
  float sh[16];
  sh_eval(rr[8], rr[9], rr[10], 3, sh);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = h == 0 ? sh[8 * (j >> 2) + (j & 3)] : sh[8 * (j >> 2) + 4 + (j & 3)];
  split_slots<8>(v, dh, dl);
}

template <bool STORE, bool FUSED, bool LW = false>
__global__ void __launch_bounds__(512) s16_small_fwd_kernel(SmallArgs a) {
  lds_load_pairs(a.wf, a.bias);
  const int lane0 = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool rmaj = FUSED && !STORE && a.ray_major;
  const int64_t ntiles = rmaj ? ((a.B + 31) >> 5) * a.n : (a.M + 31) >> 5;
  LdsPairW ws;
  for (int64_t tile0 = (int64_t)blockIdx.x * 8 + wv; tile0 < ntiles; tile0 += (int64_t)gridDim.x * 8) {
    int lane = lane0;
    asm volatile("" : "+v"(lane));        // fragment addresses are per-tile values: the LDS reads are not hoisted (spills)
    const int r = lane & 31, h = lane >> 5;
    int64_t m = tile0 * 32 + r;
    bool valid = m < a.M;
    if (rmaj) {                            // tile = (block of 32 rays, depth index): sample m = ray * n + depth
      const int64_t rb = tile0 / a.n;
      const int depth = (int)(tile0 - rb * a.n);
      int64_t ray = rb * 32 + r;
      valid = ray < a.B;
      if (!valid) ray = a.B - 1;
      m = ray * a.n + depth;
    }
    if (m >= a.M) m = a.M - 1;
    bf16x8 xh[2], xl[2], dh[1], dl[1];
    if (FUSED) {
      ngp_row_pairs<LW>(a, m, h, xh, xl, dh, dl);
    } else {
      const float* row = a.x + m * LN::CIN;
      row_pairs<s16::SplitBf16>(row, 0, h, LN::CPOS, xh[0], xl[0]); row_pairs<s16::SplitBf16>(row, 1, h, LN::CPOS, xh[1], xl[1]);
      row_pairs<s16::SplitBf16>(row + LN::CPOS, 0, h, LN::CDIR, dh[0], dl[0]);
    }
#define SINK(slot0) make_sink<STORE>(a.acts, tile0, a.astride, slot0, SM_A_LO, r, h)
#define MASK_STORE(layer) do { if (STORE) *reinterpret_cast<u32x4*>(frag_ptr(a.acts, tile0, a.astride, SM_A_MASK + (layer), r, h)) = mk; } while (0)
    if (STORE) {
      store_frags<2>(a.acts, tile0, a.astride, LN::A_X, xh, r, h); store_frags<2>(a.acts, tile0, a.astride, SM_A_LO + LN::A_X, xl, r, h);
      store_frags<1>(a.acts, tile0, a.astride, LN::A_DX, dh, r, h); store_frags<1>(a.acts, tile0, a.astride, SM_A_LO + LN::A_DX, dl, r, h);
    }
    u32x4 mk;
    bf16x8 h0h[4], h0l[4], h1h[4], h1l[4], fth[4], ftl[4];
    mk = u32x4{0u, 0u, 0u, 0u};
    s16::layer_fwd<2, 2, true, STORE>(ws, LN::F_L0, LN::BI_L0, xh, xl, h0h, h0l, mk, lane, SINK(LN::A_H0));
    MASK_STORE(0);
    mk = u32x4{0u, 0u, 0u, 0u};
    s16::layer_fwd<4, 2, true, STORE>(ws, LN::F_L1, LN::BI_L1, h0h, h0l, h1h, h1l, mk, lane, SINK(LN::A_H1));
    MASK_STORE(1);
    s16::layer_fwd<4, 2, false, false>(ws, LN::F_FA, LN::BI_FEAT, h1h, h1l, fth, ftl, mk, lane, SINK(LN::A_FEAT));     // feature: no activation
    const float alpha = s16::head<4>(ws, LN::F_FA + 8, LN::BI_ALPHA, h1h, h1l, lane)[0];
    bf16x8 hdh[2], hdl[2];
    {
      bf16x8 cth[5], ctl[5];
#pragma unroll
      for (int k = 0; k < 4; ++k) { cth[k] = fth[k]; ctl[k] = ftl[k]; }
      cth[4] = dh[0]; ctl[4] = dl[0];
      mk = u32x4{0u, 0u, 0u, 0u};
      s16::layer_fwd<5, 1, true, STORE>(ws, LN::F_DIR, LN::BI_DIR, cth, ctl, hdh, hdl, mk, lane, SINK(LN::A_HD));
      MASK_STORE(2);
    }
    const f32x16 rgb = s16::head<2>(ws, LN::F_RGB, LN::BI_RGB, hdh, hdl, lane);
    if (h == 0 && valid) {
      float4 o; o.x = rgb[0]; o.y = rgb[1]; o.z = rgb[2]; o.w = alpha;
      *reinterpret_cast<float4*>(a.out + m * 4) = o;
    }
#undef SINK
#undef MASK_STORE
  }
}

// mlp_s16x_lw.hip: launches s16_small_fwd_kernel<STORE, true, true> (a.acts selects STORE) on the filled arguments
int small_forward_lw(const SmallArgs& a, dim3 grid, hipStream_t s);

}  // namespace s16x
}  // namespace nerf
