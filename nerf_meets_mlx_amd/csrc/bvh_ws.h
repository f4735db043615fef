// The workspace of the face hierarchy (bvh.hip), carved from F alone; include/nerf_hip.h "mesh BVH".  A complete binary tree in
// heap order over nL = ceil(F / 4) leaves padded to a power of two P: the root is node 1, the children of i are 2 i and 2 i + 1,
// level l holds the nodes [2^l, 2^(l+1)), the leaves are P .. 2 P - 1 and leaf P + j holds the sorted faces 4 j .. 4 j + 3.  Node 0
// is unused and written as an empty box.  Every region starts on a multiple of 16 bytes (a pair of children is read as three
// 16-byte words).  Compiles without HIP (tests/bvh_ws_check.cpp carves it under a host compiler).
#pragma once
#include "mesh_ws.h"

namespace nerf {
namespace {

constexpr int BVH_BLOCK = 256;                      // lanes per workgroup: leaves, nodes of a level, points
constexpr int BVH_LEAF = 4;                         // sorted faces per leaf
constexpr int BVH_NODE_FLOATS = 6;                  // min x y z, max x y z
constexpr int BVH_TOP_LEVELS = 9;                   // the levels 0 .. 8 (at most 256 nodes each) are merged by one workgroup
constexpr int BVH_CELLS = 4096;                     // Morton cells per axis: 12 bits, a 36-bit code
constexpr int64_t BVH_INVALID_CODE = 1ll << 36;     // the code of an invalid face: behind every valid one
constexpr int BVH_KEY_SHIFT = 24;                   // key = code 2^24 + face

struct BvhWs {
  int64_t leaves;                                   // nL = ceil(F / 4)
  int64_t P;                                        // the smallest power of two >= max(nL, 1)
  int depth;                                        // log2 P: the level of the leaves, at most 22
  int launches;                                     // of nerf_bvh_build: the leaves, one per level above the top, the top
  float* nodes;                                     // [2 P][6]
  int32_t* order;                                   // [F] the sorted face ids, -1 for an invalid face
  int64_t bytes;
};

inline bool bvh_faces_ok(int64_t F) { return F >= 0 && F <= MESH_MAX_ITEMS; }
// the first node of level l and how many it has
inline int64_t bvh_level_first(int l) { return (int64_t)1 << l; }
inline int64_t bvh_level_nodes(int l) { return (int64_t)1 << l; }

inline BvhWs bvh_ws(void* ws, int64_t F) {
  BvhWs w;
  w.leaves = (F + BVH_LEAF - 1) / BVH_LEAF;
  w.P = 1;
  w.depth = 0;
  while (w.P < w.leaves) {
    w.P <<= 1;
    ++w.depth;
  }
  // the leaves' launch, then bvh_tree.h's tree_reduce: the internal levels depth - 1 .. 0, those below BVH_TOP_LEVELS in one launch
  w.launches = 2 + (w.depth > BVH_TOP_LEVELS ? w.depth - BVH_TOP_LEVELS : 0);
  WsCarver<16> c(ws);
  w.nodes = c.take<float>(2 * w.P * BVH_NODE_FLOATS);
  w.order = c.take<int32_t>(F);
  w.bytes = c.bytes();
  return w;
}

// what nerf_bvh_workspace_bytes returns: -1 for an F out of range
inline int64_t bvh_workspace_bytes(int64_t F) { return bvh_faces_ok(F) ? bvh_ws(nullptr, F).bytes : -1; }

}  // namespace
}  // namespace nerf
