// Stand-alone run of csrc/camera.h (host compiler, -ffp-contract=off -fsanitize=address,undefined; run by tests/test_camera_host.py,
// which compares what this prints with tests/_camera_ref.py).  Per camera (an axis-aligned one, for which zc == 0 can be hit exactly,
// and an oblique one) and point: the point, camera_point, camera_pixel and camera_nearest, floats as their bit patterns.  The points:
// 900 seeded ones in a box around the scene, 32 behind the camera, 8 on the plane zc = 0 (the first camera), 12 with a coordinate
// that is not finite, and 16 within half a pixel of each image edge on either side of it.  Then the return codes of the checks; the
// view arrays handed to camera_views_check are exactly n views long, so a read past them is an AddressSanitizer error.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

// what common.h gives the HIP units: the error text goes nowhere here
namespace nerf {
inline int fail(int code, const char*, ...) { return code; }
}
#define NERF_REQUIRE(cond, code, ...)                  \
  do {                                                 \
    if (!(cond)) return nerf::fail(code, __VA_ARGS__); \
  } while (0)
#include "../nerf_meets_mlx_amd/csrc/camera.h"

using namespace nerf;

static const int H = 48, W = 64;
static uint64_t seed = 0x9E3779B97F4A7C15ull;
static double uniform() {                                      // [0, 1)
  seed = seed * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(seed >> 11) / 9007199254740992.0;
}

static void show(int cam, const nerf_tsdf_view& vw, const float* p) {
  float c[3], u, v;
  int64_t pix = -1;
  camera_point(vw, p, c);
  camera_pixel(vw, c, &u, &v);
  const bool inside = camera_nearest(u, v, H, W, &pix);
  printf("p %d %08x %08x %08x %08x %08x %08x %08x %08x %d %lld\n", cam, float_bits(p[0]), float_bits(p[1]), float_bits(p[2]),
         float_bits(c[0]), float_bits(c[1]), float_bits(c[2]), float_bits(u), float_bits(v), (int)inside, (long long)pix);
}

// the world point at camera coordinates (xc, yc) and depth zc, up to float rounding
static void from_camera(const nerf_tsdf_view& vw, double xc, double yc, double zc, float* p) {
  const float* m = vw.c2w;
  for (int a = 0; a < 3; ++a)
    p[a] = (float)((double)m[4 * a] * xc + (double)m[4 * a + 1] * yc - (double)m[4 * a + 2] * zc + (double)m[4 * a + 3]);
}
static void from_pixel(const nerf_tsdf_view& vw, double u, double v, double zc, float* p) {
  from_camera(vw, (u - (double)vw.cx) / (double)vw.fx * zc, ((double)vw.cy - v) / (double)vw.fy * zc, zc, p);
}

static void views_case(const char* name, int n, int bad_view, int bad_number, float bad_value) {
  std::vector<nerf_tsdf_view> views((size_t)n);               // exactly n: no view past the n-th may be read
  for (int s = 0; s < n; ++s) {
    float* x = views[(size_t)s].c2w;
    for (int q = 0; q < 16; ++q) x[q] = 0.25f * (float)(q + 1) + (float)s;
    if (s == bad_view) x[bad_number] = bad_value;
  }
  CameraViews out;
  memset(&out, 0, sizeof(out));
  const int rc = camera_views_check("t", n ? views.data() : nullptr, n, &out);
  int padded = 1;
  for (int s = 0; s < CAMERA_MAX_VIEWS && rc == 0 && n > 0; ++s)
    padded = padded && memcmp(&out.v[s], &views[(size_t)(s < n ? s : 0)], sizeof(nerf_tsdf_view)) == 0;
  printf("check %s %d %d\n", name, rc, padded);
}

int main() {
  const float nan = NAN, inf = INFINITY;
  nerf_tsdf_view cams[2] = {{{1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 3.0f}, 70.0f, 70.0f, 32.0f, 24.0f},
                            {{0.6461f, -0.2449f, 0.7229f, 2.6f, 0.0f, 0.9471f, 0.3209f, 1.1f, -0.7633f, -0.2073f, 0.6119f, 2.2f},
                             66.25f, 66.5f, 31.5f, 24.25f}};
  for (int k = 0; k < 2; ++k) {
    const nerf_tsdf_view& vw = cams[k];
    float p[3];
    for (int q = 0; q < 900; ++q) {
      for (int a = 0; a < 3; ++a) p[a] = (float)(3.0 * uniform() - 1.5);
      show(k, vw, p);
    }
    for (int q = 0; q < 32; ++q) {
      from_camera(vw, 2.0 * uniform() - 1.0, 2.0 * uniform() - 1.0, -4.0 * uniform(), p);
      show(k, vw, p);
    }
    for (int q = 0; q < 8 && k == 0; ++q) {                    // q2 = p2 - t2 is exactly 0, and with it zw and zc
      p[0] = (float)(2.0 * uniform() - 1.0), p[1] = q < 2 ? 0.0f : (float)(2.0 * uniform() - 1.0), p[2] = vw.c2w[11];
      show(k, vw, p);
    }
    const float odd[4] = {nan, inf, -inf, 3.0e38f};
    for (int q = 0; q < 12; ++q) {
      for (int a = 0; a < 3; ++a) p[a] = (float)(uniform() - 0.5);
      p[q % 3] = odd[q / 3];
      show(k, vw, p);
    }
    for (int q = 0; q < 64; ++q) {                             // edge q / 16: left, right, top, bottom
      const double along = uniform(), off = uniform() - 0.5, zc = 1.0 + 3.0 * uniform();
      const int e = q / 16;
      const double u = e == 0 ? -0.5 + off : e == 1 ? (double)W - 0.5 + off : along * (double)(W - 1);
      const double v = e == 2 ? -0.5 + off : e == 3 ? (double)H - 0.5 + off : along * (double)(H - 1);
      from_pixel(vw, u, v, zc, p);
      show(k, vw, p);
    }
  }
  views_case("views_0", 0, -1, 0, 0.0f);
  views_case("views_1", 1, -1, 0, 0.0f);
  views_case("views_16", 16, -1, 0, 0.0f);
  views_case("views_1_nan", 1, 0, 0, nan);
  views_case("views_16_last_inf", 16, 15, 15, inf);
  views_case("views_3_middle_nan", 3, 1, 12, nan);
  nerf_tsdf_view one = cams[1];
  printf("check view_ok %d\n", camera_view_check("t", &one));
  printf("check view_null %d\n", camera_view_check("t", nullptr));
  for (int q = 0; q < 16; ++q) {
    one = cams[1];
    float* x = one.c2w;                                        // the 12 pose numbers, then fx, fy, cx, cy
    x[q] = q % 2 ? nan : -inf;
    printf("check view_number_%d %d\n", q, camera_view_check("t", &one));
  }
  printf("check near_ok %d %d\n", camera_near_check("t", 0.05f), camera_near_check("t", 3.0e38f));
  printf("check near_bad %d %d %d %d\n", camera_near_check("t", 0.0f), camera_near_check("t", -1.0f), camera_near_check("t", nan),
         camera_near_check("t", inf));
  printf("check image_ok %d %d %d\n", camera_image_check("t", 1, 1, CAMERA_MAX_SIDE), camera_image_check("t", CAMERA_MAX_SIDE, 1, CAMERA_MAX_SIDE),
         camera_image_check("t", 1, 4096, 4096));
  printf("check image_bad %d %d %d %d %d\n", camera_image_check("t", 0, 8, CAMERA_MAX_SIDE), camera_image_check("t", 8, 0, CAMERA_MAX_SIDE),
         camera_image_check("t", -3, 8, CAMERA_MAX_SIDE), camera_image_check("t", CAMERA_MAX_SIDE + 1, 8, CAMERA_MAX_SIDE),
         camera_image_check("t", 8, 4097, 4096));
  return 0;
}
