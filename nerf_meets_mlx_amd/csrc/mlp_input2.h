// Kernel arguments and input stage of the image-fitting model (LI) and of the 2 x 64 hash-grid model (LN), shared by their bf16
// kernels (mlp.hip) and their split-bf16 kernels (mlp_s16x.hip), beside the view model's input stage (mlp_input.h): which sample a
// lane of a 32-sample tile works on (small_tile_sample), which hash level and SH channel sits in which fragment element
// (ngp_pos_level / ngp_sh_chan), and the fused row stage that builds a sample's B fragments from rays, depths and hash tables
// (ngp_row).  As in mlp_input.h a packer says how eight floats become fragments: CvtBf16 or s16::SplitBf16.
// The maps and the tile map are integer code without a HIP dependency (tests/pack_index_check.cpp).
#pragma once
#include "mlp_arch2.h"
#include "mlp_input.h"
#if defined(__HIPCC__)
#include "hash_common.h"
#endif

namespace nerf {

// ------------------------------------------------------------------------------------------
// fused 2 x 64 query: channel c of the position input is feature c & 1 of hash level c >> 1 (16 levels x 2 features), so lane half
// h owns levels 8 ks + 4 (j >> 2) + 2 h + ((j & 3) >> 1) of k-step ks: the two lanes of a sample split the levels between them;
// SH degree 3 = 16 channels = one k-step
// ------------------------------------------------------------------------------------------
__host__ __device__ constexpr int ngp_pos_level(int ks, int h, int j) { return 8 * ks + 4 * (j >> 2) + 2 * h + ((j & 3) >> 1); }
__host__ __device__ constexpr int ngp_sh_chan(int h, int j) { return 8 * (j >> 2) + 4 * h + (j & 3); }
__host__ __device__ constexpr bool ngp_channels_are_kperm() {
  for (int h = 0; h < 2; ++h)
    for (int j = 0; j < 8; ++j) {
      for (int ks = 0; ks < 2; ++ks)
        if (kperm(ks, h, j) != 2 * ngp_pos_level(ks, h, j) + (j & 1)) return false;
      if (kperm(0, h, j) != ngp_sh_chan(h, j)) return false;
    }
  return true;
}
static_assert(ngp_channels_are_kperm(), "element j of lane half h: position channel kperm(ks, h, j) = (level, feature j & 1); SH channel kperm(0, h, j)");

// Sample of lane r of tile `tile0` of the 2 x 64 forward kernels, and whether the lane owns it (else: a clamped duplicate whose
// result is not written).  Sample-major: 32 consecutive samples.  Ray-major (fused inference only): ONE depth index of 32
// ADJACENT RAYS: neighbouring pixels' samples at the same depth are 0.0012 apart in the unit cube, so the 32 lanes of a gather
// instruction fall into the same or adjacent cells at every level below N_l ~ 800 (13 of 16), where 32 consecutive depths of one
// ray (0.021 apart) share cells only below N_l ~ 48.  Same values per sample.  a: anything with M = B n, B and n.
struct TileSample { int64_t m; bool valid; };
template <class A>
NERF_IN TileSample small_tile_sample(const A& a, int64_t tile0, int r, bool rmaj) {
  int64_t m = tile0 * 32 + r;
  bool valid = m < a.M;
  if (rmaj) {                              // tile = (block of 32 rays, depth index): sample m = ray * n + depth
    const int64_t rb = tile0 / a.n;
    const int depth = (int)(tile0 - rb * a.n);
    int64_t ray = rb * 32 + r;
    valid = ray < a.B;
    if (!valid) ray = a.B - 1;
    m = ray * a.n + depth;
  }
  if (m >= a.M) m = a.M - 1;
  return TileSample{m, valid};
}
// ... and the rule and the tile count that go with it: ray-major needs a full block of rays and keeps no activations
template <class A>
NERF_IN int64_t small_tiles(const A& a) { return a.ray_major ? ((a.B + 31) >> 5) * a.n : (a.M + 31) >> 5; }
NERF_IN bool small_ray_major(bool train, int option, int64_t B) { return !train && option && B >= 32; }

#if defined(__HIPCC__)
struct ImgArgs {
  const bf16x8* wf; const bf16x8* wb; const float* bias;
  const float* x;        // [M,40] embedded rows
  const float* d_out;    // [M,out_ch]
  int64_t M; int out_ch;
  float* out;            // [M,out_ch]
  void* acts; void* dz;
  int64_t astride, zstride;
};

struct SmallArgs {
  const bf16x8* wf; const bf16x8* wb; const float* bias;
  const float* x;        // [M,48]: 32 position features | 16 direction features
  const float* d_raw;    // [M,4]
  int64_t M;
  float* out;            // [M,4] raw
  float* d_x;            // [M,32] dL/d(position features) or nullptr
  void* acts; void* dz;
  int64_t astride, zstride;
  // fused configs[4] query: rows are computed in the kernel from rays / depths / hash tables (16 levels x 2 features)
  const float* rays; const float* z; int n; const float* tables; uint32_t T; ResTab rt; float pos_scale, pos_offset;
  // fp16 shadow image of the tables (one 4-byte pair per entry) or nullptr: gathered instead of `tables`.  bf16 kernels only: the
  // split-bf16 ones gather the float32 master tables (reference tolerance), and a precision-22 query leaves this null
  const uint32_t* tables_h;
  int ray_major; int64_t B;      // small_tile_sample
  // per-level weights of nerf_ngp_query_fused_lw, read by the LW kernels only (last member: the other kernels' argument
  // offsets are what they were)
  LevelTab lw;
};

// B fragments of one sample straight from the hash tables and the view direction -> PK::pack(values, out[k]...) for k = position
// k-steps 0, 1 and the direction k-step (2): every `out` is an array of three fragments.  Interpolated values stay float32 until
// they are packed.  HALF: gathers from the fp16 shadow tables.  LW: value = w[l] * interpolation in float32, ahead of the packing;
// w[l] == 0: the lane's gathers of that level are predicated off (h selects the levels, so the predicate differs within a wave)
// and the value is +0.
template <bool HALF, bool LW, class PK, class... OUT>
__device__ __forceinline__ void ngp_row(const SmallArgs& a, int64_t m, int h, OUT&... out) {
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
    for (int j = 0; j < 8; j += 2) {
      const int l = ngp_pos_level(ks, 0, j) + 2 * h;
      const Corners c = corners_of(px, py, pz, a.rt.res[l], mask);
      FeatVec<2> fv;
      if (LW) {
        const float w = h ? a.lw.w[ngp_pos_level(ks, 1, j)] : a.lw.w[ngp_pos_level(ks, 0, j)];       // two scalars and a select
        fv = hash_level_lw<HALF>(a.tables + (size_t)l * a.T * 2, a.tables_h + (size_t)l * a.T, c, w);
      } else {
        fv = HALF ? hash_level_h(a.tables_h + (size_t)l * a.T, c) : hash_level<2>(a.tables + (size_t)l * a.T * 2, c);
      }
      v[j] = fv.v[0];
      v[j + 1] = fv.v[1];
    }
    PK::pack(v, out[ks]...);
  }
  float sh[16];
  sh_eval(rr[8], rr[9], rr[10], 3, sh);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = h == 0 ? sh[ngp_sh_chan(0, j)] : sh[ngp_sh_chan(1, j)];
  PK::pack(v, out[2]...);
}
// the same three fragments of an already-encoded row x[m][48]
template <class PK, class... OUT>
__device__ __forceinline__ void small_row(const float* __restrict__ row, int h, OUT&... out) {
  row_pairs<PK>(row, 0, h, LN::CPOS, out[0]...);
  row_pairs<PK>(row, 1, h, LN::CPOS, out[1]...);
  row_pairs<PK>(row + LN::CPOS, 0, h, LN::CDIR, out[2]...);
}
#endif

}  // namespace nerf
