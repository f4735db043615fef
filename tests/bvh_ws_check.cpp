// Stand-alone run of csrc/bvh_ws.h (host compiler, -fsanitize=address,undefined; run by tests/test_bvh_host.py): the workspace of
// the face hierarchy carved for a few F, every region as its offset from the base and its size in bytes, the tree's shape and the
// levels' node ranges, then what an F out of range gives.
#include <stdint.h>
#include <stdio.h>

#include "../nerf_meets_mlx_amd/csrc/bvh_ws.h"

using namespace nerf;

static void carve(int64_t F) {
  alignas(16) static char base[16];
  const BvhWs w = bvh_ws(base, F);
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(base);
  auto at = [p0](const void* p) { return (long long)(reinterpret_cast<uintptr_t>(p) - p0); };
  printf("ws %lld bytes %lld total %lld leaves %lld P %lld depth %d launches %d\n", (long long)F, (long long)w.bytes,
         (long long)bvh_workspace_bytes(F), (long long)w.leaves, (long long)w.P, w.depth, w.launches);
  printf("region nodes %lld %lld\n", at(w.nodes), (long long)(2 * w.P * BVH_NODE_FLOATS * 4));
  printf("region order %lld %lld\n", at(w.order), (long long)(F * 4));
  // the levels tile the nodes [1, 2 P) without a gap, the leaves last; every leaf slot of a face lies below 2 P
  int64_t next = 1;
  for (int l = 0; l <= w.depth; ++l) {
    if (bvh_level_first(l) != next) printf("gap at level %d\n", l);
    next = bvh_level_first(l) + bvh_level_nodes(l);
  }
  printf("tiled %d last_leaf %lld\n", (int)(next == 2 * w.P && bvh_level_first(w.depth) == w.P),
         (long long)(F > 0 ? w.P + (F - 1) / BVH_LEAF : -1));
}

int main() {
  const int64_t top = 1ll << 24;
  const int64_t sizes[5] = {0, 1, 4, 5, top};
  for (const int64_t F : sizes) carve(F);
  printf("bad %lld %lld %lld\n", (long long)bvh_workspace_bytes(-1), (long long)bvh_workspace_bytes(top + 1),
         (long long)bvh_workspace_bytes(INT64_MAX));
  printf("consts %d %d %d %d %lld %d\n", BVH_LEAF, BVH_NODE_FLOATS, BVH_TOP_LEVELS, BVH_CELLS, (long long)BVH_INVALID_CODE,
         BVH_KEY_SHIFT);
  return 0;
}
