// The projective texture bake (project.hip), the one statement in code of include/nerf_hip.h "view-projected texture": what one
// posed image says about one texel of the atlas of texture.h.
//   texel    position x and unit normal n of tex_point at the texel's barycentrics (texture.h: the texel of nerf_texture_rows)
//   camera   camera.h: camera_point; !(zc >= near): none; after the facing test camera_pixel
//   facing   e = t - x; L = sqrt((e0 e0 + e1 e1) + e2 e2); cosv = ((n0 e0 + n1 e1) + n2 e2) / L; !(cosv >= cos_min): none; w = cosv
//   visible  camera.h: camera_nearest, the pixel the rasteriser drew; outside: none.  a = acc[pix], s = depth[pix]; a or s NaN, or
//            a < acc_min: none.  ez = s / a - zc; !(ez >= 0 - depth_tol): none
//   colour   x0 = floorf(u), y0 = floorf(v); unless 0 <= x0, x0 + 1 <= W - 1, 0 <= y0, y0 + 1 <= H - 1 (floats): none.
//            fx = u - x0, fy = v - y0, gx = 1 - fx, gy = 1 - fy; w00 = gx gy, w10 = fx gy, w01 = gx fy, w11 = fx fy (the first index
//            along x); c = ((w00 c00 + w10 c10) + w01 c01) + w11 c11 per channel; a NaN channel: none
//   fold     blend: S_c = S_c + w c, S_w = S_w + w.  best: if w > S_w then S = (c, w)
// The argument checks compile without HIP (tests/project_check.cpp runs them under a host compiler with sanitizers).
#pragma once
#include "camera.h"
#include "texture.h"

namespace nerf {
namespace {

constexpr int PROJECT_BLOCK = 256;

// what every view of a launch shares
struct ProjectRule {
  int H, W, mode;
  float near, neg_tol, cos_min, acc_min;
};

inline int project_mode_check(const char* who, int mode) {
  NERF_REQUIRE(mode == NERF_PROJECT_BLEND || mode == NERF_PROJECT_BEST, NERF_E_SHAPE, "%s: mode must be %d (blend) or %d (best), got %d",
               who, NERF_PROJECT_BLEND, NERF_PROJECT_BEST, mode);
  return NERF_OK;
}

// every argument of nerf_project_accumulate; fills the layout, the rule and the views.  *work: whether anything is to be launched
inline int project_accumulate_check(const char* who, const float* verts, const float* normals, int64_t V, const int32_t* faces, int64_t F,
                                    int T, int64_t p0, int64_t count, const nerf_tsdf_view* views_host, int n, int H, int W,
                                    const float* images, const float* depth, const float* acc, float near, float depth_tol,
                                    float cos_min, float acc_min, int mode, const float* state, TexLayout* lay, ProjectRule* rule,
                                    CameraViews* views, bool* work) {
  *work = false;
  int rc = tex_mesh_check(who, V, F, T, lay);
  if (!rc) rc = tex_chunk_check(who, *lay, p0, count);
  if (!rc) rc = project_mode_check(who, mode);
  if (rc) return rc;
  NERF_REQUIRE(n >= 0 && n <= NERF_PROJECT_MAX_VIEWS, NERF_E_SHAPE, "%s: need 0 <= n <= %d views (got %d)", who, NERF_PROJECT_MAX_VIEWS, n);
  rc = camera_image_check(who, H, W, CAMERA_MAX_SIDE);
  if (!rc) rc = camera_near_check(who, near);
  if (rc) return rc;
  NERF_REQUIRE(std::isfinite(depth_tol) && depth_tol >= 0.0f, NERF_E_SHAPE, "%s: depth_tol must be finite and >= 0 (got %g)", who,
               (double)depth_tol);
  NERF_REQUIRE(cos_min > 0.0f && cos_min <= 1.0f, NERF_E_SHAPE, "%s: need 0 < cos_min <= 1 (got %g)", who, (double)cos_min);
  NERF_REQUIRE(acc_min > 0.0f && acc_min <= 1.0f, NERF_E_SHAPE, "%s: need 0 < acc_min <= 1 (got %g)", who, (double)acc_min);
  NERF_REQUIRE(n == 0 || views_host, NERF_E_NULL, "%s: NULL views", who);
  rc = camera_views_check(who, views_host, n, views);
  if (rc) return rc;
  *rule = ProjectRule{H, W, mode, near, 0.0f - depth_tol, cos_min, acc_min};
  if (n == 0 || count == 0) return NERF_OK;
  NERF_REQUIRE(images && depth && acc && state && (faces || F == 0) && ((verts && normals) || V == 0), NERF_E_NULL, "%s: NULL pointer", who);
  NERF_REQUIRE(((uintptr_t)state & 15) == 0, NERF_E_SHAPE, "%s: state must be 16-byte aligned", who);
  *work = true;
  return NERF_OK;
}

// every argument of nerf_project_finish
inline int project_finish_check(const char* who, const float* state, int64_t F, int T, int64_t p0, int64_t count, int mode,
                                const uint8_t* image, const uint8_t* seen, TexLayout* lay, bool* work) {
  *work = false;
  int rc = tex_layout(who, F, T, lay);
  if (!rc) rc = tex_chunk_check(who, *lay, p0, count);
  if (!rc) rc = project_mode_check(who, mode);
  if (rc) return rc;
  if (count == 0) return NERF_OK;
  NERF_REQUIRE(state && image && seen, NERF_E_NULL, "%s: NULL pointer", who);
  NERF_REQUIRE(((uintptr_t)state & 15) == 0, NERF_E_SHAPE, "%s: state must be 16-byte aligned", who);
  *work = true;
  return NERF_OK;
}

#if defined(__HIPCC__)
// what the view (its camera, its image [H, W, 3] and its depth / acc maps [H W]) says about the texel at x with the normal n:
// false for no observation, else the weight and the colour
__device__ __forceinline__ bool project_observe(const nerf_tsdf_view& vw, const ProjectRule& r, const float* __restrict__ image,
                                                const float* __restrict__ depth, const float* __restrict__ acc, const float* x,
                                                const float* n, float* w, float* c) {
  float cam[3], u, v;
  camera_point(vw, x, cam);
  const float zc = cam[2];
  if (!(zc >= r.near)) return false;                                       // in front of the near plane, behind the camera, or NaN
  const float e0 = vw.c2w[3] - x[0], e1 = vw.c2w[7] - x[1], e2 = vw.c2w[11] - x[2];
  const float dot = (n[0] * e0 + n[1] * e1) + n[2] * e2;
#if PROJECT_SIGN_FIRST
  // measured, not shipped: cos_min > 0 and L >= 0, so a dot product that is not positive fails the facing
  // test whatever L is; leaving here spares the back half of the mesh the square root and the division.  Same bits.
  if (!(dot > 0.0f)) return false;
#endif
  const float L = sqrt_rn((e0 * e0 + e1 * e1) + e2 * e2);
  const float cosv = div_rn(dot, L);
  if (!(cosv >= r.cos_min)) return false;                                  // facing away, grazing, no normal, or NaN
  camera_pixel(vw, cam, &u, &v);
  int64_t pix;
  if (!camera_nearest(u, v, r.H, r.W, &pix)) return false;                 // outside the image, or not finite
  const float fW = (float)r.W, fH = (float)r.H;
  const float a = acc[pix], s = depth[pix];
  if (a != a || s != s || a < r.acc_min) return false;
  const float ez = div_rn(s, a) - zc;
  if (!(ez >= r.neg_tol)) return false;                                    // behind what the view sees, or NaN
  const float x0 = floorf(u), y0 = floorf(v);
  if (!(x0 >= 0.0f && x0 + 1.0f <= fW - 1.0f && y0 >= 0.0f && y0 + 1.0f <= fH - 1.0f)) return false;
  const float fx = u - x0, fy = v - y0;
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  const float w00 = gx * gy, w10 = fx * gy, w01 = gx * fy, w11 = fx * fy;
  const float* t00 = image + 3 * ((int64_t)(int)y0 * r.W + (int)x0);
  const float* t01 = t00 + 3 * (int64_t)r.W;
  bool ok = true;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    c[ch] = ((w00 * t00[ch] + w10 * t00[3 + ch]) + w01 * t01[ch]) + w11 * t01[3 + ch];
    ok = ok && c[ch] == c[ch];
  }
  *w = cosv;
  return ok;
}
#endif

}  // namespace
}  // namespace nerf
