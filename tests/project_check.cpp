// Stand-alone run of csrc/project.h's host parts (host compiler, -fsanitize=address,undefined; run by tests/test_project_host.py):
// the argument checks of nerf_project_accumulate and nerf_project_finish, which are these two functions and nothing else, on good
// and bad arguments.  The view array handed over is exactly n views long, so a read past it is an AddressSanitizer error; the
// device pointers are never dereferenced.  Prints "name rc work" per case.
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
#include "../nerf_meets_mlx_amd/csrc/project.h"

using namespace nerf;

struct Acc {
  const float* verts = (const float*)4096;
  const float* normals = (const float*)4096;
  int64_t V = 10;
  const int32_t* faces = (const int32_t*)4096;
  int64_t F = 9;
  int T = 8;
  int64_t p0 = 0, count = 5;
  int n = 2, H = 48, W = 64;
  const float* images = (const float*)4096;
  const float* depth = (const float*)4096;
  const float* acc = (const float*)4096;
  float near = 0.5f, tol = 0.01f, cos_min = 0.1f, acc_min = 0.5f;
  int mode = NERF_PROJECT_BLEND;
  const float* state = (const float*)4096;
  bool null_views = false;
  int bad_view = -1, bad_number = 0;
  float bad_value = NAN;
};

static void run(const char* name, const Acc& a) {
  std::vector<nerf_tsdf_view> views((size_t)(a.n > 0 && a.n <= 64 ? a.n : 0));        // exactly n: no view past the n-th may be read
  for (size_t s = 0; s < views.size(); ++s) {
    float* x = views[s].c2w;
    for (int q = 0; q < 16; ++q) x[q] = 0.25f * (float)(q + 1) + (float)s;
    if ((int)s == a.bad_view) x[a.bad_number] = a.bad_value;
  }
  TexLayout lay;
  ProjectRule rule;
  CameraViews out;
  memset(&out, 0, sizeof(out));
  bool work = true;
  const int rc = project_accumulate_check("t", a.verts, a.normals, a.V, a.faces, a.F, a.T, a.p0, a.count,
                                          a.null_views || views.empty() ? nullptr : views.data(), a.n, a.H, a.W, a.images, a.depth, a.acc,
                                          a.near, a.tol, a.cos_min, a.acc_min, a.mode, a.state, &lay, &rule, &out, &work);
  int copied = 1;
  if (rc == 0 && a.n > 0)
    for (int s = 0; s < NERF_PROJECT_MAX_VIEWS; ++s) copied = copied && memcmp(&out.v[s], &views[s < a.n ? s : 0], sizeof(nerf_tsdf_view)) == 0;
  printf("%s %d %d %d\n", name, rc, (int)work, copied);
}

struct Fin {
  const float* state = (const float*)4096;
  int64_t F = 9;
  int T = 8;
  int64_t p0 = 0, count = 5;
  int mode = NERF_PROJECT_BEST;
  const uint8_t* image = (const uint8_t*)4096;
  const uint8_t* seen = (const uint8_t*)4096;
};

static void run(const char* name, const Fin& a) {
  TexLayout lay;
  bool work = true;
  const int rc = project_finish_check("t", a.state, a.F, a.T, a.p0, a.count, a.mode, a.image, a.seen, &lay, &work);
  printf("%s %d %d 1\n", name, rc, (int)work);
}

#define CASE(kind, name, ...) \
  do {                        \
    kind a;                   \
    __VA_ARGS__;              \
    run(name, a);             \
  } while (0)

int main() {
  const int64_t P = 30 * 20;                                  // 9 faces at T = 8: 5 cells of side 10, 3 a row, 2 rows
  const float inf = INFINITY, nan = NAN;
  CASE(Acc, "ok.acc_good");
  CASE(Acc, "ok.acc_one_view", a.n = 1);
  CASE(Acc, "ok.acc_16_views", a.n = 16);
  CASE(Acc, "ok.acc_whole_atlas", a.count = P);
  CASE(Acc, "ok.acc_best", a.mode = NERF_PROJECT_BEST);
  CASE(Acc, "ok.acc_limits", a.H = 16384; a.W = 1; a.cos_min = 1.0f; a.acc_min = 1.0f; a.tol = 0.0f);
  CASE(Acc, "idle.acc_no_views", a.n = 0; a.images = nullptr; a.depth = nullptr; a.acc = nullptr; a.state = nullptr);
  CASE(Acc, "idle.acc_no_texels", a.count = 0; a.state = nullptr; a.images = nullptr);
  CASE(Acc, "idle.acc_end_of_atlas", a.p0 = P; a.count = 0);
  CASE(Acc, "shape.acc_n_negative", a.n = -1);
  CASE(Acc, "shape.acc_n_17", a.n = 17);
  CASE(Acc, "shape.acc_H_0", a.H = 0);
  CASE(Acc, "shape.acc_W_0", a.W = 0);
  CASE(Acc, "shape.acc_H_16385", a.H = 16385);
  CASE(Acc, "shape.acc_W_16385", a.W = 16385);
  CASE(Acc, "shape.acc_H_negative", a.H = -3);
  CASE(Acc, "shape.acc_T_1", a.T = 1);
  CASE(Acc, "shape.acc_T_65", a.T = 65);
  CASE(Acc, "shape.acc_F_negative", a.F = -1);
  CASE(Acc, "shape.acc_F_large", a.F = ((int64_t)1 << 24) + 1);
  CASE(Acc, "shape.acc_atlas_too_wide", a.F = (int64_t)1 << 24);
  CASE(Acc, "shape.acc_V_negative", a.V = -1);
  CASE(Acc, "shape.acc_V_large", a.V = ((int64_t)1 << 24) + 1);
  CASE(Acc, "shape.acc_near_0", a.near = 0.0f);
  CASE(Acc, "shape.acc_near_negative", a.near = -1.0f);
  CASE(Acc, "shape.acc_near_inf", a.near = inf);
  CASE(Acc, "shape.acc_near_nan", a.near = nan);
  CASE(Acc, "shape.acc_tol_negative", a.tol = -0.001f);
  CASE(Acc, "shape.acc_tol_inf", a.tol = inf);
  CASE(Acc, "shape.acc_tol_nan", a.tol = nan);
  CASE(Acc, "shape.acc_cos_0", a.cos_min = 0.0f);
  CASE(Acc, "shape.acc_cos_above_1", a.cos_min = 1.5f);
  CASE(Acc, "shape.acc_cos_nan", a.cos_min = nan);
  CASE(Acc, "shape.acc_accmin_0", a.acc_min = 0.0f);
  CASE(Acc, "shape.acc_accmin_above_1", a.acc_min = 1.0001f);
  CASE(Acc, "shape.acc_accmin_nan", a.acc_min = nan);
  CASE(Acc, "shape.acc_mode_2", a.mode = 2);
  CASE(Acc, "shape.acc_mode_negative", a.mode = -1);
  CASE(Acc, "shape.acc_p0_negative", a.p0 = -1);
  CASE(Acc, "shape.acc_count_negative", a.count = -1);
  CASE(Acc, "shape.acc_chunk_past_end", a.p0 = P - 4);
  CASE(Acc, "shape.acc_chunk_overflow", a.p0 = (int64_t)1 << 62; a.count = (int64_t)1 << 62);
  CASE(Acc, "shape.acc_state_unaligned", a.state = (const float*)4100);
  for (int q = 0; q < 16; ++q) {
    char name[64];
    snprintf(name, sizeof(name), "shape.acc_view1_number%d_nan", q);
    CASE(Acc, name, a.bad_view = 1; a.bad_number = q);
  }
  CASE(Acc, "shape.acc_view0_inf", a.bad_view = 0; a.bad_number = 12; a.bad_value = inf);
  CASE(Acc, "shape.acc_view15_inf", a.n = 16; a.bad_view = 15; a.bad_number = 3; a.bad_value = -inf);
  CASE(Acc, "null.acc_views", a.null_views = true);
  CASE(Acc, "null.acc_verts", a.verts = nullptr);
  CASE(Acc, "null.acc_normals", a.normals = nullptr);
  CASE(Acc, "null.acc_faces", a.faces = nullptr);
  CASE(Acc, "null.acc_images", a.images = nullptr);
  CASE(Acc, "null.acc_depth", a.depth = nullptr);
  CASE(Acc, "null.acc_acc", a.acc = nullptr);
  CASE(Acc, "null.acc_state", a.state = nullptr);
  CASE(Fin, "ok.fin_good");
  CASE(Fin, "ok.fin_blend_whole", a.mode = NERF_PROJECT_BLEND; a.count = P);
  CASE(Fin, "idle.fin_no_texels", a.count = 0; a.state = nullptr; a.image = nullptr; a.seen = nullptr);
  CASE(Fin, "shape.fin_T_1", a.T = 1);
  CASE(Fin, "shape.fin_T_65", a.T = 65);
  CASE(Fin, "shape.fin_F_negative", a.F = -1);
  CASE(Fin, "shape.fin_atlas_too_wide", a.F = (int64_t)1 << 24);
  CASE(Fin, "shape.fin_mode_2", a.mode = 2);
  CASE(Fin, "shape.fin_p0_negative", a.p0 = -1);
  CASE(Fin, "shape.fin_count_negative", a.count = -1);
  CASE(Fin, "shape.fin_chunk_past_end", a.p0 = P; a.count = 1);
  CASE(Fin, "shape.fin_state_unaligned", a.state = (const float*)4104);
  CASE(Fin, "null.fin_state", a.state = nullptr);
  CASE(Fin, "null.fin_image", a.image = nullptr);
  CASE(Fin, "null.fin_seen", a.seen = nullptr);
  return 0;
}
