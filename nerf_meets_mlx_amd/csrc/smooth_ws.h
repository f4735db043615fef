// The workspace of the mesh smoother (smooth.hip), carved from (V, F) alone; include/nerf_hip.h "mesh smoothing".  Everything whose
// size depends on V only comes first, so that nerf_smooth_run and nerf_smooth_normals, which are not told F, find their regions
// from V; the entries, 3 F of them at most, come last.  Every region starts on a multiple of 8 bytes.  Compiles without HIP
// (tests/smooth_ws_check.cpp carves it under a host compiler).
#pragma once
#include <stdint.h>

namespace nerf {
namespace {

constexpr int SMOOTH_BLOCK = 256;                   // vertices (or faces) per workgroup
constexpr int64_t SMOOTH_MAX_ITEMS = 1ll << 24;     // V, F: 3 F entries fit an int

struct SmoothEntry {                                // one face at one of its corners: the other two, in face order
  int32_t b, c;
};

struct SmoothWs {
  int64_t nblk_v;
  int64_t* blk;                                     // [nblk_v] entries per workgroup of vertices, scanned in place
  int64_t* total;                                   // [1] entries in all
  float* tmp;                                       // [V][3] the other side of the ping-pong
  int32_t* off;                                     // [V + 1] first entry of a row; off[V] = total
  int32_t* cur;                                     // [V] entries of a row, then its fill cursor
  SmoothEntry* ent;                                 // [3 F]
  int64_t bytes;
};

inline bool smooth_sizes_ok(int64_t V, int64_t F) { return V >= 0 && V <= SMOOTH_MAX_ITEMS && F >= 0 && F <= SMOOTH_MAX_ITEMS; }
inline int64_t smooth_blocks(int64_t n) { return (n + SMOOTH_BLOCK - 1) / SMOOTH_BLOCK; }

inline SmoothWs smooth_ws(void* ws, int64_t V, int64_t F) {
  SmoothWs w;
  w.nblk_v = smooth_blocks(V);
  uintptr_t p = reinterpret_cast<uintptr_t>(ws);
  const uintptr_t p0 = p;
  auto take = [&p](int64_t bytes) {
    const uintptr_t at = p;
    p += (uintptr_t)((bytes + 7) & ~(int64_t)7);
    return at;
  };
  w.blk = reinterpret_cast<int64_t*>(take(w.nblk_v * 8));
  w.total = reinterpret_cast<int64_t*>(take(8));
  w.tmp = reinterpret_cast<float*>(take(V * 12));
  w.off = reinterpret_cast<int32_t*>(take((V + 1) * 4));
  w.cur = reinterpret_cast<int32_t*>(take(V * 4));
  w.ent = reinterpret_cast<SmoothEntry*>(take(3 * F * 8));
  w.bytes = (int64_t)(p - p0);
  return w;
}

// what nerf_smooth_workspace_bytes returns: -1 for sizes out of range
inline int64_t smooth_workspace_bytes(int64_t V, int64_t F) { return smooth_sizes_ok(V, F) ? smooth_ws(nullptr, V, F).bytes : -1; }

}  // namespace
}  // namespace nerf
