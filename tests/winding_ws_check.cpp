// Stand-alone run of csrc/winding_ws.h (host compiler, -fsanitize=address,undefined; run by tests/test_winding_host.py): the
// workspace of the winding-number moments carved for a few F, its region as the offset from the base and its size in bytes, the
// tree's shape as the hierarchy's own carve gives it, then what an F out of range gives.
#include <stdint.h>
#include <stdio.h>

#include "../nerf_meets_mlx_amd/csrc/winding_ws.h"

using namespace nerf;

static void carve(int64_t F) {
  alignas(16) static char base[16];
  const WindWs w = wind_ws(base, F);
  const BvhWs b = bvh_ws(base, F);
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(base);
  printf("ws %lld bytes %lld total %lld P %lld depth %d launches %d bvh_P %lld bvh_depth %d bvh_launches %d\n", (long long)F,
         (long long)w.bytes, (long long)wind_workspace_bytes(F), (long long)w.P, w.depth, w.launches, (long long)b.P, b.depth,
         b.launches);
  printf("region moments %lld %lld\n", (long long)(reinterpret_cast<uintptr_t>(w.moments) - p0),
         (long long)(2 * w.P * WIND_NODE_DOUBLES * 8));
  // the record of the last node ends inside the region
  printf("last_record_end %lld\n", (long long)((2 * w.P - 1) * WIND_NODE_DOUBLES * 8 + WIND_NODE_DOUBLES * 8));
}

int main() {
  const int64_t top = 1ll << 24;
  const int64_t sizes[5] = {0, 1, 4, 5, top};
  for (const int64_t F : sizes) carve(F);
  printf("bad %lld %lld %lld\n", (long long)wind_workspace_bytes(-1), (long long)wind_workspace_bytes(top + 1),
         (long long)wind_workspace_bytes(INT64_MAX));
  printf("consts %d %d %d %d %d %d\n", WIND_NODE_DOUBLES, WIND_N, WIND_C, WIND_R, WIND_A, WIND_S);
  return 0;
}
