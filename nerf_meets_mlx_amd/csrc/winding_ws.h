// The workspace of the winding-number moments (winding.hip), carved from F alone; include/nerf_hip.h "mesh winding number".  One
// record of WIND_NODE_DOUBLES float64 per node of the face hierarchy (bvh_ws.h: heap order, the root is node 1, 2 P nodes), 96 bytes,
// so every record starts on a multiple of 16 bytes:
//   [0..2] N   the sum of the faces' area vectors          [3..5] c   the area-weighted centroid S / A (or the box midpoint)
//   [6]    r   from c to the farthest corner of the box    [7]    A   the sum of the faces' areas
//   [8..10] S  the sum of area times centroid              [11]   0
// The query reads the first seven; A and S are what a parent adds up.  Compiles without HIP (tests/winding_ws_check.cpp carves it
// under a host compiler).
#pragma once
#include "bvh_ws.h"

namespace nerf {
namespace {

constexpr int WIND_NODE_DOUBLES = 12;
constexpr int WIND_N = 0, WIND_C = 3, WIND_R = 6, WIND_A = 7, WIND_S = 8;

struct WindWs {
  int64_t P;                                        // the hierarchy's: leaves padded to a power of two
  int depth;                                        // log2 P
  int launches;                                     // of nerf_winding_build: the hierarchy's count, the same function of F
  double* moments;                                  // [2 P][12]
  int64_t bytes;
};

inline WindWs wind_ws(void* ws, int64_t F) {
  const BvhWs b = bvh_ws(nullptr, F);
  WindWs w;
  w.P = b.P;
  w.depth = b.depth;
  w.launches = b.launches;
  w.moments = reinterpret_cast<double*>(ws);
  w.bytes = (2 * w.P * WIND_NODE_DOUBLES * 8 + 15) & ~(int64_t)15;
  return w;
}

// what nerf_winding_workspace_bytes returns: -1 for an F out of range
inline int64_t wind_workspace_bytes(int64_t F) { return bvh_faces_ok(F) ? wind_ws(nullptr, F).bytes : -1; }

}  // namespace
}  // namespace nerf
