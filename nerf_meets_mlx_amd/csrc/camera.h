// The pinhole camera of the surface and fusion kernels (tsdf.hip, raster.hip, project.hip, mip.hip), the one statement in code of
// include/nerf_hip.h "pinhole camera":
//   view     nerf_tsdf_view, 16 finite floats: c2w [3, 4] row-major = [R | t] (the camera looks along its -z, +y is up in the image),
//            then fx, fy, cx, cy
//   point    q = p - t; (xc, yc, zw) = R^T q, each sum associated as (r0 q0 + r1 q1) + r2 q2; zc = 0 - zw, the depth along the
//            optical axis.  Every operation rounds to float32 on its own (-ffp-contract=off).
//   pixel    u = fx (xc / zc) + cx, v = cy - fy (yc / zc), the divisions div_rn; pixel (px, py) has its centre at (u, v) = (px, py)
//   nearest  fu = floorf(u + 0.5f), fv likewise; inside iff 0 <= fu < W and 0 <= fv < H, tested on the floats before the cast (NaN
//            and +-inf fail); the pixel index is fv W + fu (int64)
//   views    a launch takes up to CAMERA_MAX_VIEWS views by value (scalar loads, uniform over the launch); the unused slots repeat
//            view 0, so no slot is ever wild
// The whole header compiles without HIP (tests/camera_check.cpp runs it under a host compiler, which supplies nerf::fail and
// NERF_REQUIRE itself).  Not here, on purpose: the order of the tests around these steps (TSDF and the bake test zc before they
// divide, the rasteriser divides first and tests after), the NaN tests on what a map holds at the pixel, the rasteriser's snap
// and guard band (raster.h), and the bilinear weights of the bake (project.h) and of the atlas (texture.h).
#pragma once
#include "lattice.h"

namespace nerf {
namespace {

constexpr int CAMERA_MAX_VIEWS = 16;
constexpr int CAMERA_MAX_SIDE = 16384;                         // height and width of a drawn or baked image

struct CameraViews { nerf_tsdf_view v[CAMERA_MAX_VIEWS]; };
static_assert(sizeof(nerf_tsdf_view) == 16 * sizeof(float), "16 floats per view");
static_assert(NERF_TSDF_MAX_VIEWS == CAMERA_MAX_VIEWS && NERF_PROJECT_MAX_VIEWS == CAMERA_MAX_VIEWS, "one padded array for both");

// world point p -> c = (xc, yc, zc)
__host__ __device__ __forceinline__ void camera_point(const nerf_tsdf_view& vw, const float* p, float* c) {
  const float q0 = p[0] - vw.c2w[3], q1 = p[1] - vw.c2w[7], q2 = p[2] - vw.c2w[11];
  c[0] = (vw.c2w[0] * q0 + vw.c2w[4] * q1) + vw.c2w[8] * q2;
  c[1] = (vw.c2w[1] * q0 + vw.c2w[5] * q1) + vw.c2w[9] * q2;
  const float zw = (vw.c2w[2] * q0 + vw.c2w[6] * q1) + vw.c2w[10] * q2;
  c[2] = 0.0f - zw;
}

// c = (xc, yc, zc) -> (u, v); the caller decides whether zc is tested before or after
__host__ __device__ __forceinline__ void camera_pixel(const nerf_tsdf_view& vw, const float* c, float* u, float* v) {
  *u = vw.fx * div_rn(c[0], c[2]) + vw.cx;
  *v = vw.cy - vw.fy * div_rn(c[1], c[2]);
}

// the pixel of an H x W map nearest to (u, v): false outside the map or for a coordinate that is not finite, else its index
__host__ __device__ __forceinline__ bool camera_nearest(float u, float v, int H, int W, int64_t* pix) {
  const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
  *pix = 0;                                                    // (outside: defined all the same)
  if (!(fu >= 0.0f && fu < (float)W && fv >= 0.0f && fv < (float)H)) return false;
  *pix = (int64_t)(int)fv * W + (int)fu;
  return true;
}

inline int camera_near_check(const char* who, float near) {
  NERF_REQUIRE(std::isfinite(near) && near > 0.0f, NERF_E_SHAPE, "%s: near must be finite and > 0 (got %g)", who, (double)near);
  return NERF_OK;
}
inline int camera_image_check(const char* who, int H, int W, int max_side) {
  NERF_REQUIRE(H >= 1 && W >= 1 && H <= max_side && W <= max_side, NERF_E_SHAPE, "%s: need 1 <= H, W <= %d (got %d x %d)", who, max_side,
               H, W);
  return NERF_OK;
}
inline int camera_view_check(const char* who, const nerf_tsdf_view* view) {
  NERF_REQUIRE(view, NERF_E_NULL, "%s: NULL view", who);
  const float* x = view->c2w;                                  // the 12 pose numbers, then fx, fy, cx, cy
  for (int q = 0; q < 16; ++q) NERF_REQUIRE(std::isfinite(x[q]), NERF_E_SHAPE, "%s: non-finite camera number %d", who, q);
  return NERF_OK;
}
// n views of the caller's (0 <= n <= CAMERA_MAX_VIEWS, non-NULL unless n = 0; at most n are read) into the padded array
inline int camera_views_check(const char* who, const nerf_tsdf_view* views, int n, CameraViews* out) {
  for (int s = 0; s < CAMERA_MAX_VIEWS && n > 0; ++s) {
    out->v[s] = views[s < n ? s : 0];
    if (s >= n) continue;
    const float* x = out->v[s].c2w;
    for (int q = 0; q < 16; ++q) NERF_REQUIRE(std::isfinite(x[q]), NERF_E_SHAPE, "%s: view %d: non-finite camera number %d", who, s, q);
  }
  return NERF_OK;
}

}  // namespace
}  // namespace nerf
