// Projective texture bake: the texels of a mesh's atlas coloured from posed images, each observation kept only where the mesh's own
// depth map of that view says the texel is visible (a shadow-map test).  Semantics in include/nerf_hip.h "view-projected texture",
// the rule in code in project.h; tests/_project_ref.py reproduces every output bit for bit.  No reference counterpart.  No
// workspace, no host read, and every output element has one writer.
//   accumulate  one lane per texel of a chunk of the atlas in raster order.  The lane finds its point and normal once (texture.h, the
//               texel of the rows kernel), loads its 16 B of state in one access, folds up to NERF_PROJECT_MAX_VIEWS views into it
//               in registers, in order, and stores it in one access: 32 B of state per texel cross HBM per launch and not per view.
//               Per view and texel the gathers are two map reads and four corners of three floats; the view parameters are kernel
//               arguments (scalar loads, uniform over the launch).  Identical to one launch per view in the same order.
//   finish      one lane per texel: one 16-byte load, three byte stores and the seen flag.
#include "project.h"

namespace nerf {
namespace {

// ---- accumulate: per texel 12 B of face indices and 72 B of corners gathered (cache hits), 16 B read and written; per view and
// texel that passes the camera and facing tests 8 B of maps and 48 B of image gathered
__global__ void __launch_bounds__(PROJECT_BLOCK) project_accumulate_kernel(const float* __restrict__ verts, const float* __restrict__ normals,
                                                                          int V, const int* __restrict__ faces, TexLayout lay, int64_t p0,
                                                                          int64_t count, CameraViews views, int n, ProjectRule rule,
                                                                          const float* __restrict__ images, const float* __restrict__ depth,
                                                                          const float* __restrict__ acc, float4* __restrict__ state) {
  const int64_t q = (int64_t)blockIdx.x * PROJECT_BLOCK + threadIdx.x;
  if (q >= count) return;
  const int64_t p = p0 + q;
  int g[3];
  float wb, wc;
  if (!tex_texel(lay, faces, V, p, g, &wb, &wc)) return;                   // a texel of no face, or of a bad one: no observation
  float x[3], nr[3];
  tex_point(verts, normals, g, wb, wc, x, nr);
  float4 S = state[p];
  const int64_t HW = (int64_t)rule.H * rule.W;
  for (int s = 0; s < n; ++s) {
    float w, c[3];
    if (!project_observe(views.v[s], rule, images + 3 * (s * HW), depth + s * HW, acc + s * HW, x, nr, &w, c)) continue;
    if (rule.mode == NERF_PROJECT_BLEND) {
      S.x = S.x + w * c[0];
      S.y = S.y + w * c[1];
      S.z = S.z + w * c[2];
      S.w = S.w + w;
    } else if (w > S.w) {                                                  // strict: of equal weights the earlier view stays
      S = make_float4(c[0], c[1], c[2], w);
    }
  }
  state[p] = S;
}

// ---- finish: per texel 16 B read in one load, 3 B of the fallback read, 4 B written
__global__ void __launch_bounds__(PROJECT_BLOCK) project_finish_kernel(const float4* __restrict__ state, int64_t p0, int64_t count, int mode,
                                                                      const uint8_t* __restrict__ fallback, uint8_t* __restrict__ image,
                                                                      uint8_t* __restrict__ seen) {
  const int64_t q = (int64_t)blockIdx.x * PROJECT_BLOCK + threadIdx.x;
  if (q >= count) return;
  const int64_t p = p0 + q;
  const float4 S = state[p];
  const bool got = S.w > 0.0f;                                             // (NaN: not seen)
  const float c[3] = {S.x, S.y, S.z};
  uint8_t b[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {                                         // both sides of the choice, so that S stays one 16-byte load
    const uint8_t mine = (uint8_t)rintf(255.0f * tex_unit(mode == NERF_PROJECT_BLEND ? div_rn(c[ch], S.w) : c[ch]));
    const uint8_t other = fallback ? fallback[3 * p + ch] : (uint8_t)0;
    b[ch] = got ? mine : other;
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) image[3 * p + ch] = b[ch];
  seen[p] = got ? 1 : 0;
}

}  // namespace
}  // namespace nerf

using namespace nerf;

extern "C" int nerf_project_accumulate(const float* verts, const float* normals, int64_t V, const int32_t* faces, int64_t F, int texels,
                                       int64_t p0, int64_t count, const nerf_tsdf_view* views_host, int n, int H, int W,
                                       const float* images, const float* depth, const float* acc, float near, float depth_tol,
                                       float cos_min, float acc_min, int mode, float* state, void* stream) {
  const char* who = "nerf_project_accumulate";
  TexLayout lay;
  ProjectRule rule;
  CameraViews views;
  bool work;
  const int rc = project_accumulate_check(who, verts, normals, V, faces, F, texels, p0, count, views_host, n, H, W, images, depth, acc,
                                          near, depth_tol, cos_min, acc_min, mode, state, &lay, &rule, &views, &work);
  if (rc || !work) return rc;
  NERF_LAUNCH(who, project_accumulate_kernel, blocks(count, PROJECT_BLOCK), PROJECT_BLOCK, as_stream(stream), verts, normals, (int)V, faces, lay, p0,
              count, views, n, rule, images, depth, acc, reinterpret_cast<float4*>(state));
  return NERF_OK;
}

extern "C" int nerf_project_finish(const float* state, int64_t F, int texels, int64_t p0, int64_t count, int mode,
                                   const uint8_t* fallback, uint8_t* image, uint8_t* seen, void* stream) {
  const char* who = "nerf_project_finish";
  TexLayout lay;
  bool work;
  const int rc = project_finish_check(who, state, F, texels, p0, count, mode, image, seen, &lay, &work);
  if (rc || !work) return rc;
  NERF_LAUNCH(who, project_finish_kernel, blocks(count, PROJECT_BLOCK), PROJECT_BLOCK, as_stream(stream), reinterpret_cast<const float4*>(state), p0,
              count, mode, fallback, image, seen);
  return NERF_OK;
}
