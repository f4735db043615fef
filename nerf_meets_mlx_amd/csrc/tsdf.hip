// TSDF fusion of rendered depth / opacity maps into a truncated signed distance volume on the mesh-extraction lattice
// (KinectFusion; nerfstudio's TSDF export).  Semantics in include/nerf_hip.h "TSDF fusion"; tests/_tsdf_ref.py reproduces every
// output bit for bit.  No reference counterpart.  The lattice, its box and its cell centres are lattice.h's, the camera and the
// nearest pixel of a map camera.h's.  One lane per voxel: a lane loads its D, Wt and flags once, folds up to NERF_TSDF_MAX_VIEWS
// views into them in registers, in order, and stores once -- 18 B of state per voxel cross HBM per launch and not per view; the
// maps (4 B per pixel each) are gathered, and at 16 views of 800 x 800 those gathers, not the state, are most of the launch time
// (DESIGN.md section 21).  The view parameters are kernel arguments (scalar loads, uniform over the launch).  Every voxel has one
// writer and the views are folded in call order: bit-reproducible, and identical to one launch per view.
#include "camera.h"

namespace nerf {
namespace {

__global__ void __launch_bounds__(LATTICE_BLOCK) tsdf_reset_kernel(float* __restrict__ D, float* __restrict__ Wt,
                                                               uint8_t* __restrict__ flags, int64_t n3) {
  const int64_t p = lattice_lane();
  if (p >= n3) return;
  D[p] = 0.0f;
  Wt[p] = 0.0f;
  flags[p] = 0;
}

// ---- integrate: 4 + 4 + 1 B read and written per voxel and launch; per view and voxel at most two gathered map reads.
__global__ void __launch_bounds__(LATTICE_BLOCK) tsdf_integrate_kernel(float* __restrict__ D, float* __restrict__ Wt,
                                                                   uint8_t* __restrict__ flags, Lattice bx, CameraViews views,
                                                                   int n, int H, int W, const float* __restrict__ depth,
                                                                   const float* __restrict__ acc, float tau, float acc_min,
                                                                   float far, int carve) {
  const int64_t lg = lattice_lane();
  if (lg >= lattice_n3(bx.R)) return;
  int c[3];
  lattice_coords((int)lg, bx.R, c);
  float p[3];
  lattice_centre(bx, c, p);                                                // bit for bit the points of marching cubes
  float d_mean = D[lg], wt = Wt[lg];
  const uint8_t f_in = flags[lg];
  uint8_t f = f_in;
  const float neg_tau = 0.0f - tau;
  const int64_t HW = (int64_t)H * W;
  for (int s = 0; s < n; ++s) {
    float cam[3], u, v;
    camera_point(views.v[s], p, cam);
    const float zc = cam[2];
    if (!(zc > 0.0f)) continue;                                            // behind the camera, or NaN
    camera_pixel(views.v[s], cam, &u, &v);
    int64_t pix;
    if (!camera_nearest(u, v, H, W, &pix)) continue;                       // outside the image, or not finite
    pix += s * HW;
    const float a = acc[pix], sd = depth[pix];
    if (a != a || sd != sd) continue;
    float d;
    if (a < acc_min) {
      if (!(carve && zc <= far)) continue;
      d = 1.0f;                                                            // a ray that hits nothing: empty all along it
    } else {
      const float e = div_rn(sd, a) - zc;
      if (e < neg_tau) {
        f |= 1;                                                            // behind a surface by more than the truncation
        continue;
      }
      if (!(e >= neg_tau)) continue;                                       // NaN
      d = fminf(1.0f, div_rn(e, tau));
    }
    const float wn = wt + 1.0f;
    d_mean = div_rn(d_mean * wt + d, wn);
    wt = wn;
  }
  D[lg] = d_mean;
  Wt[lg] = wt;
  if (f != f_in) flags[lg] = f;
}

// ---- finish: 9 B read, 4 B written per voxel.
__global__ void __launch_bounds__(LATTICE_BLOCK) tsdf_volume_kernel(const float* __restrict__ D, const float* __restrict__ Wt,
                                                                const uint8_t* __restrict__ flags, int64_t n3, float min_views,
                                                                float* __restrict__ vol) {
  const int64_t p = lattice_lane();
  if (p >= n3) return;
  float v;
  if (Wt[p] >= min_views) v = 0.0f - D[p];
  else v = (flags[p] & 1) ? 1.0f : -1.0f;
  vol[p] = v;
}

}  // namespace
}  // namespace nerf

using namespace nerf;

extern "C" int nerf_tsdf_reset(float* D, float* Wt, uint8_t* flags, int res, void* stream) {
  int rc = lattice_res_check("nerf_tsdf_reset", res);
  if (rc) return rc;
  NERF_REQUIRE(D && Wt && flags, NERF_E_NULL, "nerf_tsdf_reset: NULL pointer");
  hipLaunchKernelGGL(tsdf_reset_kernel, dim3(lattice_blocks(res)), dim3(LATTICE_BLOCK), 0, as_stream(stream), D, Wt, flags,
                     lattice_n3(res));
  return check_launch("nerf_tsdf_reset");
}

extern "C" int nerf_tsdf_integrate(float* D, float* Wt, uint8_t* flags, int res, const float* lo, const float* hi,
                                   const nerf_tsdf_view* views_host, int n, int H, int W, const float* depth, const float* acc,
                                   float trunc, float acc_min, float far, int carve, void* stream) {
  const char* who = "nerf_tsdf_integrate";
  int rc = lattice_res_check(who, res);
  if (rc) return rc;
  Lattice bx;
  rc = lattice_box(who, res, lo, hi, &bx);
  if (rc) return rc;
  NERF_REQUIRE(n >= 0 && n <= NERF_TSDF_MAX_VIEWS, NERF_E_SHAPE, "%s: need 0 <= n <= %d views (got %d)", who, NERF_TSDF_MAX_VIEWS, n);
  // (float)H and (float)W are exact up to 2^24, and n H W then stays far inside int64
  NERF_REQUIRE(H > 0 && W > 0 && H <= (1 << 24) && W <= (1 << 24), NERF_E_SHAPE, "%s: need 1 <= H, W <= 2^24 (got %d x %d)", who, H, W);
  NERF_REQUIRE(std::isfinite(trunc) && trunc > 0.0f, NERF_E_SHAPE, "%s: trunc must be finite and > 0 (got %g)", who, (double)trunc);
  NERF_REQUIRE(std::isfinite(far) && far > 0.0f, NERF_E_SHAPE, "%s: far must be finite and > 0 (got %g)", who, (double)far);
  NERF_REQUIRE(acc_min > 0.0f && acc_min <= 1.0f, NERF_E_SHAPE, "%s: need 0 < acc_min <= 1 (got %g)", who, (double)acc_min);
  NERF_REQUIRE(carve == 0 || carve == 1, NERF_E_SHAPE, "%s: carve must be 0 or 1 (got %d)", who, carve);
  NERF_REQUIRE(D && Wt && flags, NERF_E_NULL, "%s: NULL state pointer", who);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(views_host && depth && acc, NERF_E_NULL, "%s: NULL views / depth / acc", who);
  CameraViews views;
  rc = camera_views_check(who, views_host, n, &views);
  if (rc) return rc;
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(lattice_blocks(res)), dim3(LATTICE_BLOCK), 0, as_stream(stream), D, Wt, flags, bx,
                     views, n, H, W, depth, acc, trunc, acc_min, far, carve);
  return check_launch(who);
}

extern "C" int nerf_tsdf_volume(const float* D, const float* Wt, const uint8_t* flags, int res, int min_views, float* vol_out,
                                void* stream) {
  int rc = lattice_res_check("nerf_tsdf_volume", res);
  if (rc) return rc;
  NERF_REQUIRE(min_views >= 1, NERF_E_SHAPE, "nerf_tsdf_volume: need min_views >= 1 (got %d)", min_views);
  NERF_REQUIRE(D && Wt && flags && vol_out, NERF_E_NULL, "nerf_tsdf_volume: NULL pointer");
  hipLaunchKernelGGL(tsdf_volume_kernel, dim3(lattice_blocks(res)), dim3(LATTICE_BLOCK), 0, as_stream(stream), D, Wt, flags,
                     lattice_n3(res), (float)min_views, vol_out);
  return check_launch("nerf_tsdf_volume");
}
