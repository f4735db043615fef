// A mip pyramid for the texture atlas of texture.hip, a level of detail per face from its footprint on the screen, and the trilinear
// lookup through both.  Semantics in include/nerf_hip.h "texture mip pyramid", stated in code in mip.h; tests/_mip_ref.py reproduces
// every output bit for bit.  No reference counterpart.  No atomics, no host read, no workspace: every output element has one writer.
//   reduce   one lane per texel of a chunk of the coarse atlas in raster order.  An in-triangle lane takes nine bilinear lookups
//            of the fine level (36 gathered texels, cache hits: the nine footprints overlap and a face's lanes are neighbours); a
//            gutter lane recomputes the three or seven in-triangle bytes its extrapolation needs rather than wait for a
//            second launch, so a level is one launch and no lane reads what another writes.  Three byte stores per lane, as the
//            store of texture.hip (packing them measured slower there).
//   lod      one lane per face: the rasteriser's own setup (12 B of indices, 36 B of vertices gathered), 4 B written.
//   sample   one lane per surface sample: 12 B read (16 B with a lod per sample), one or two bilinear lookups, 12 B written.  The
//            levels arrive by value; a lane selects its level's pointer and layout with compares against constant indices, so the
//            argument block is never indexed by a lane's own number and nothing goes to scratch.
#include "mip.h"

namespace nerf {
namespace {

__global__ void __launch_bounds__(MIP_BLOCK) mip_reduce_kernel(const uint8_t* __restrict__ fine, TexLayout lf, TexLayout lc, int64_t p0,
                                                              int64_t count, uint8_t* __restrict__ coarse) {
  const int64_t q = (int64_t)blockIdx.x * MIP_BLOCK + threadIdx.x;
  if (q >= count) return;
  const int64_t p = p0 + q;
  const int Y = (int)(p / lc.W), X = (int)(p - (int64_t)Y * lc.W);
  int i, j, b[3] = {0, 0, 0};
  const int f = tex_owner(lc, X, Y, &i, &j);
  if (f < lc.F) mip_texel(fine, lf, lc.T, f, i, j, b);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) coarse[3 * p + ch] = (uint8_t)b[ch];
}

__global__ void __launch_bounds__(MIP_BLOCK) mip_lod_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                           nerf_tsdf_view view, float near, MipChain chain, float scale,
                                                           float* __restrict__ lod) {
  const int f = blockIdx.x * MIP_BLOCK + threadIdx.x;
  if (f >= F) return;
  RasterFace rf;
  float out = 0.0f;
  if (raster_setup(verts, V, faces + 3 * (int64_t)f, view, near, 0, &rf) == RASTER_OK) {
    const int64_t D = raster_edge(rf.X[0], rf.Y[0], rf.X[1], rf.Y[1], rf.X[2], rf.Y[2]);
    out = mip_lod(chain, D < 0 ? -D : D, scale);
  }
  lod[f] = out;
}

__global__ void __launch_bounds__(MIP_BLOCK) mip_sample_kernel(MipLevels lv, const int* __restrict__ sface, const float* __restrict__ bary,
                                                              const float* __restrict__ lod, int per_face, int64_t n,
                                                              float* __restrict__ rgb) {
  const int64_t s = (int64_t)blockIdx.x * MIP_BLOCK + threadIdx.x;
  if (s >= n) return;
  const int f = sface[s];
  float out[3] = {0.0f, 0.0f, 0.0f};
  if (f >= 0 && f < lv.lay[0].F) {
    const float wb = tex_unit(bary[2 * s]);
    const float hi = 1.0f - wb;
    float wc = tex_pos(bary[2 * s + 1]);
    wc = wc < hi ? wc : hi;
    float lam = tex_pos(lod[per_face ? (int64_t)f : s]);       // NaN -> 0
    const float top = (float)(lv.L - 1);
    lam = lam < top ? lam : top;
    const int l = (int)floorf(lam);
    const float t = lam - (float)l;
    const uint8_t* im0 = lv.image[0];
    const uint8_t* im1 = lv.image[0];
    TexLayout l0 = lv.lay[0], l1 = lv.lay[0];
#pragma unroll
    for (int k = 1; k < NERF_MIP_MAX_LEVELS; ++k) {
      if (k == l) { im0 = lv.image[k]; l0 = lv.lay[k]; }
      if (k == l + 1) { im1 = lv.image[k]; l1 = lv.lay[k]; }
    }
    const float d0 = (float)(l0.T - 1);
    tex_lookup(im0, l0, f, wb * d0, wc * d0, out);
    if (t != 0.0f) {                                           // (then l + 1 <= L - 1)
      float c1[3];
      const float d1 = (float)(l1.T - 1), u = 1.0f - t;
      tex_lookup(im1, l1, f, wb * d1, wc * d1, c1);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) out[ch] = (u * out[ch]) + (t * c1[ch]);
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) rgb[3 * s + ch] = out[ch];
}

}  // namespace
}  // namespace nerf

using namespace nerf;

extern "C" int nerf_mip_levels(int texels, int32_t* out) {
  const int rc = mip_texels_check("nerf_mip_levels", texels);
  if (rc) return rc;
  NERF_REQUIRE(out, NERF_E_NULL, "nerf_mip_levels: NULL out");
  int chain[NERF_MIP_MAX_LEVELS];
  const int L = mip_chain(texels, chain);
  out[0] = L;
  for (int l = 0; l < NERF_MIP_MAX_LEVELS; ++l) out[1 + l] = l < L ? chain[l] : 0;
  return NERF_OK;
}

extern "C" int nerf_mip_reduce(const uint8_t* fine, int64_t F, int texels_fine, uint8_t* coarse, int64_t p0, int64_t count, void* stream) {
  TexLayout lf, lc;
  bool work;
  const int rc = mip_reduce_check("nerf_mip_reduce", fine, F, texels_fine, coarse, p0, count, &lf, &lc, &work);
  if (rc || !work) return rc;
  NERF_LAUNCH("nerf_mip_reduce", mip_reduce_kernel, blocks(count, MIP_BLOCK), MIP_BLOCK, as_stream(stream), fine, lf, lc, p0, count, coarse);
  return NERF_OK;
}

extern "C" int nerf_mip_lod(const float* verts, int64_t V, const int32_t* faces, int64_t F, const nerf_tsdf_view* view_host, float near,
                            int texels, float scale, float* lod, void* stream) {
  MipChain chain;
  bool work;
  const int rc = mip_lod_check("nerf_mip_lod", verts, V, faces, F, view_host, near, texels, scale, lod, &chain, &work);
  if (rc || !work) return rc;
  NERF_LAUNCH("nerf_mip_lod", mip_lod_kernel, blocks(F, MIP_BLOCK), MIP_BLOCK, as_stream(stream), verts, (int)V, faces, (int)F, *view_host, near,
              chain, scale, lod);
  return NERF_OK;
}

extern "C" int nerf_mip_sample(const uint8_t* const* images_host, int64_t F, int texels, const int32_t* face, const float* bary,
                               const float* lod, int per_face, int64_t n, float* rgb, void* stream) {
  MipLevels lv;
  bool work;
  const int rc = mip_sample_check("nerf_mip_sample", images_host, F, texels, face, bary, lod, per_face, n, rgb, &lv, &work);
  if (rc || !work) return rc;
  NERF_LAUNCH("nerf_mip_sample", mip_sample_kernel, blocks(n, MIP_BLOCK), MIP_BLOCK, as_stream(stream), lv, face, bary, lod, per_face, n, rgb);
  return NERF_OK;
}
