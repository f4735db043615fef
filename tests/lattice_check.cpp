// Stand-alone run of csrc/lattice.h's host parts (host compiler, -fsanitize=address,undefined; run by tests/test_lattice_host.py,
// which compares what this prints with tests/_mesh_ref.py).  Per R in {2, 3, 65, 512} over one non-cubic box: h, lattice_blocks,
// and for the first, the last and 1000 seeded linear indices the coordinates of lattice_coords and the centre of lattice_centre,
// floats as their bit patterns.  Then the return codes of the three checks on good and bad arguments.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

// what common.h gives the HIP units: the error text goes nowhere here
namespace nerf {
inline int fail(int code, const char*, ...) { return code; }
}
#define NERF_REQUIRE(cond, code, ...)                  \
  do {                                                 \
    if (!(cond)) return nerf::fail(code, __VA_ARGS__); \
  } while (0)
#include "../nerf_meets_mlx_amd/csrc/lattice.h"

using namespace nerf;

static void point(const Lattice& lat, int64_t l) {
  int c[3];
  float p[3];
  lattice_coords((int)l, lat.R, c);
  lattice_centre(lat, c, p);
  printf("p %lld %d %d %d %08x %08x %08x\n", (long long)l, c[0], c[1], c[2], float_bits(p[0]), float_bits(p[1]), float_bits(p[2]));
}

int main() {
  const float lo[3] = {-1.5f, -0.7f, 0.1f}, hi[3] = {1.5f, 2.3f, 0.35f};
  const int sizes[4] = {2, 3, 65, 512};
  for (int R : sizes) {
    Lattice lat;
    const int rc = lattice_box("lattice_check", R, lo, hi, &lat);
    const int64_t n3 = lattice_n3(R);
    printf("R %d rc %d n3 %lld blocks %u\n", R, rc, (long long)n3, lattice_blocks(R));
    printf("h %08x %08x %08x\n", float_bits(lat.h[0]), float_bits(lat.h[1]), float_bits(lat.h[2]));
    point(lat, 0);
    point(lat, n3 - 1);
    uint64_t s = 0x9E3779B97F4A7C15ull + (uint64_t)R;
    for (int q = 0; q < 1000; ++q) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      point(lat, (int64_t)((s >> 33) % (uint64_t)n3));
    }
  }
  Lattice lat;
  const float nan = NAN, inf = INFINITY;
  printf("check res_ok %d %d %d %d\n", lattice_res_check("t", 2), lattice_res_check("t", 512), lattice_check("t", 2, 0.25f),
         lattice_box("t", 2, lo, hi, &lat));
  printf("check res_1 %d %d %d\n", lattice_res_check("t", 1), lattice_check("t", 1, 0.0f), (int)lattice_res_ok(1));
  printf("check res_513 %d %d %d\n", lattice_res_check("t", 513), lattice_check("t", 513, 0.0f), (int)lattice_res_ok(513));
  printf("check iso_nan %d\n", lattice_check("t", 2, nan));
  printf("check iso_inf %d %d\n", lattice_check("t", 2, inf), lattice_check("t", 2, -inf));
  for (int a = 0; a < 3; ++a) {
    float l2[3] = {lo[0], lo[1], lo[2]}, h2[3] = {hi[0], hi[1], hi[2]};
    h2[a] = l2[a];
    printf("check box_equal_%d %d\n", a, lattice_box("t", 2, l2, h2, &lat));
    h2[a] = l2[a] - 1.0f;
    printf("check box_reversed_%d %d\n", a, lattice_box("t", 2, l2, h2, &lat));
    h2[a] = hi[a];
    l2[a] = nan;
    printf("check box_nan_lo_%d %d\n", a, lattice_box("t", 2, l2, h2, &lat));
    l2[a] = lo[a];
    h2[a] = nan;
    printf("check box_nan_hi_%d %d\n", a, lattice_box("t", 2, l2, h2, &lat));
  }
  printf("check box_null %d\n", lattice_box("t", 2, nullptr, hi, &lat));
  return 0;
}
