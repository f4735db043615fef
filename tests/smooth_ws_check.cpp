// Stand-alone run of csrc/smooth_ws.h (host compiler, -fsanitize=address,undefined; run by tests/test_smooth_host.py): the
// workspace of the mesh smoother carved for a few (V, F), every region as its offset from the base and its size in bytes, then
// what sizes out of range give.
#include <stdint.h>
#include <stdio.h>

#include "../nerf_meets_mlx_amd/csrc/smooth_ws.h"

using namespace nerf;

static void carve(int64_t V, int64_t F) {
  alignas(8) static char base[8];
  const SmoothWs w = smooth_ws(base, V, F);
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(base);
  auto at = [p0](const void* p) { return (long long)(reinterpret_cast<uintptr_t>(p) - p0); };
  printf("ws %lld %lld bytes %lld total %lld nblk %lld\n", (long long)V, (long long)F, (long long)w.bytes,
         (long long)smooth_workspace_bytes(V, F), (long long)w.nblk_v);
  printf("region blk %lld %lld\n", at(w.blk), (long long)(w.nblk_v * 8));
  printf("region total %lld %lld\n", at(w.total), 8ll);
  printf("region tmp %lld %lld\n", at(w.tmp), (long long)(V * 12));
  printf("region off %lld %lld\n", at(w.off), (long long)((V + 1) * 4));
  printf("region cur %lld %lld\n", at(w.cur), (long long)(V * 4));
  printf("region ent %lld %lld\n", at(w.ent), (long long)(3 * F * (int64_t)sizeof(SmoothEntry)));
  // run and normals carve with F = 0: everything but the size must agree
  const SmoothWs r = smooth_ws(base, V, 0);
  printf("same %d\n", (int)(r.blk == w.blk && r.total == w.total && r.tmp == w.tmp && r.off == w.off && r.cur == w.cur && r.ent == w.ent));
}

int main() {
  const int64_t top = 1ll << 24;
  const int64_t sizes[5][2] = {{0, 0}, {1, 1}, {4, 4}, {257, 511}, {top, top}};
  for (const auto& s : sizes) carve(s[0], s[1]);
  printf("bad %lld %lld %lld %lld %lld\n", (long long)smooth_workspace_bytes(-1, 0), (long long)smooth_workspace_bytes(0, -1),
         (long long)smooth_workspace_bytes(top + 1, 0), (long long)smooth_workspace_bytes(0, top + 1),
         (long long)smooth_workspace_bytes(INT64_MAX, INT64_MAX));
  printf("entry %d\n", (int)sizeof(SmoothEntry));
  return 0;
}
