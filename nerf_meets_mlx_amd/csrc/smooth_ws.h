// The workspace of the mesh smoother (smooth.hip), carved from (V, F) alone; include/nerf_hip.h "mesh smoothing".  Everything whose
// size depends on V only comes first, so that nerf_smooth_run and nerf_smooth_normals, which are not told F, find their regions
// from V; the entries, 3 F of them at most, come last.  Every region starts on a multiple of 8 bytes.  Compiles without HIP
// (tests/smooth_ws_check.cpp carves it under a host compiler).
#pragma once
#include "mesh_ws.h"

namespace nerf {
namespace {

constexpr int SMOOTH_BLOCK = 256;                   // vertices (or faces) per workgroup

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

inline bool smooth_sizes_ok(int64_t V, int64_t F) { return V >= 0 && V <= MESH_MAX_ITEMS && F >= 0 && F <= MESH_MAX_ITEMS; }

inline SmoothWs smooth_ws(void* ws, int64_t V, int64_t F) {
  SmoothWs w;
  w.nblk_v = mesh_blocks(V, SMOOTH_BLOCK);
  WsCarver<8> c(ws);
  w.blk = c.take<int64_t>(w.nblk_v);
  w.total = c.take<int64_t>(1);
  w.tmp = c.take<float>(V * 3);
  w.off = c.take<int32_t>(V + 1);
  w.cur = c.take<int32_t>(V);
  w.ent = c.take<SmoothEntry>(3 * F);
  w.bytes = c.bytes();
  return w;
}

// what nerf_smooth_workspace_bytes returns: -1 for sizes out of range
inline int64_t smooth_workspace_bytes(int64_t V, int64_t F) { return smooth_sizes_ok(V, F) ? smooth_ws(nullptr, V, F).bytes : -1; }

}  // namespace
}  // namespace nerf
