// The projective texture bake (project.hip), the one statement in code of include/nerf_hip.h "view-projected texture": what one
// posed image says about one texel of the atlas of texture.h.
//   texel    position x and unit normal n of tex_point at the texel's barycentrics (texture.h: the texel of nerf_texture_rows)
//   camera   nerf_tsdf_view, as raster.h: q = x - t; (xc, yc, zw) = R^T q with the sums associated as in tsdf_integrate_kernel;
//            zc = 0 - zw; !(zc >= near): none.  u = fx (xc / zc) + cx, v = cy - fy (yc / zc)
//   facing   e = t - x; L = sqrt((e0 e0 + e1 e1) + e2 e2); cosv = ((n0 e0 + n1 e1) + n2 e2) / L; !(cosv >= cos_min): none; w = cosv
//   visible  fu = floorf(u + 0.5f), fv likewise; unless 0 <= fu < W and 0 <= fv < H (floats): none.  a = acc[fv W + fu],
//            s = depth[fv W + fu]; a or s NaN, or a < acc_min: none.  ez = s / a - zc; !(ez >= 0 - depth_tol): none
//   colour   x0 = floorf(u), y0 = floorf(v); unless 0 <= x0, x0 + 1 <= W - 1, 0 <= y0, y0 + 1 <= H - 1 (floats): none.
//            fx = u - x0, fy = v - y0, gx = 1 - fx, gy = 1 - fy; w00 = gx gy, w10 = fx gy, w01 = gx fy, w11 = fx fy (the first index
//            along x); c = ((w00 c00 + w10 c10) + w01 c01) + w11 c11 per channel; a NaN channel: none
//   fold     blend: S_c = S_c + w c, S_w = S_w + w.  best: if w > S_w then S = (c, w)
// The argument checks compile without HIP (tests/project_check.cpp runs them under a host compiler with sanitizers).
#pragma once
#include "texture.h"

namespace nerf {
namespace {

constexpr int PROJECT_BLOCK = 256;
constexpr int PROJECT_MAX_SIDE = 16384;

struct ProjectViews {
  nerf_tsdf_view v[NERF_PROJECT_MAX_VIEWS];
};
static_assert(sizeof(nerf_tsdf_view) == 16 * sizeof(float), "16 floats per view");

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
                                    ProjectViews* views, bool* work) {
  *work = false;
  int rc = tex_mesh_check(who, V, F, T, lay);
  if (!rc) rc = tex_chunk_check(who, *lay, p0, count);
  if (!rc) rc = project_mode_check(who, mode);
  if (rc) return rc;
  NERF_REQUIRE(n >= 0 && n <= NERF_PROJECT_MAX_VIEWS, NERF_E_SHAPE, "%s: need 0 <= n <= %d views (got %d)", who, NERF_PROJECT_MAX_VIEWS, n);
  NERF_REQUIRE(H >= 1 && W >= 1 && H <= PROJECT_MAX_SIDE && W <= PROJECT_MAX_SIDE, NERF_E_SHAPE, "%s: need 1 <= H, W <= %d (got %d x %d)",
               who, PROJECT_MAX_SIDE, H, W);
  NERF_REQUIRE(std::isfinite(near) && near > 0.0f, NERF_E_SHAPE, "%s: near must be finite and > 0 (got %g)", who, (double)near);
  NERF_REQUIRE(std::isfinite(depth_tol) && depth_tol >= 0.0f, NERF_E_SHAPE, "%s: depth_tol must be finite and >= 0 (got %g)", who,
               (double)depth_tol);
  NERF_REQUIRE(cos_min > 0.0f && cos_min <= 1.0f, NERF_E_SHAPE, "%s: need 0 < cos_min <= 1 (got %g)", who, (double)cos_min);
  NERF_REQUIRE(acc_min > 0.0f && acc_min <= 1.0f, NERF_E_SHAPE, "%s: need 0 < acc_min <= 1 (got %g)", who, (double)acc_min);
  NERF_REQUIRE(n == 0 || views_host, NERF_E_NULL, "%s: NULL views", who);
  for (int s = 0; s < NERF_PROJECT_MAX_VIEWS; ++s) {
    if (n == 0) break;
    views->v[s] = views_host[s < n ? s : 0];
    if (s >= n) continue;
    const float* x = views->v[s].c2w;                        // the 12 pose numbers, then fx, fy, cx, cy
    for (int q = 0; q < 16; ++q) NERF_REQUIRE(std::isfinite(x[q]), NERF_E_SHAPE, "%s: view %d: non-finite camera number %d", who, s, q);
  }
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
  const float q0 = x[0] - vw.c2w[3], q1 = x[1] - vw.c2w[7], q2 = x[2] - vw.c2w[11];
  const float xc = (vw.c2w[0] * q0 + vw.c2w[4] * q1) + vw.c2w[8] * q2;
  const float yc = (vw.c2w[1] * q0 + vw.c2w[5] * q1) + vw.c2w[9] * q2;
  const float zw = (vw.c2w[2] * q0 + vw.c2w[6] * q1) + vw.c2w[10] * q2;
  const float zc = 0.0f - zw;
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
  const float u = vw.fx * div_rn(xc, zc) + vw.cx;
  const float v = vw.cy - vw.fy * div_rn(yc, zc);
  const float fW = (float)r.W, fH = (float)r.H;
  const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
  if (!(fu >= 0.0f && fu < fW && fv >= 0.0f && fv < fH)) return false;     // outside the image, or not finite: before the cast
  const int64_t pix = (int64_t)(int)fv * r.W + (int)fu;
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
