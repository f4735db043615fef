// What the units on the face hierarchy share (bvh.hip's boxes, winding.hip's moments) beyond its layout (bvh_ws.h, which compiles
// without HIP): the bottom-up pass over the heap-ordered tree and the walk over a leaf's faces.  The pass takes an Op, a small struct
// by value: merge(i) makes node i from its children 2 i and 2 i + 1, which the pass has completed, and unused(lane) writes the
// record of the unused node 0 from the first lanes of the last workgroup.  No workgroup waits for another; no atomic, no LDS.
#pragma once
#include "bvh_ws.h"
#include "distance.h"

namespace nerf {
namespace {

static_assert(BVH_BLOCK == DIST_BLOCK, "DIST_LAUNCH launches the hierarchy's kernels");

// ---- one level [first, 2 first): one lane per node
template <class Op>
__global__ void __launch_bounds__(BVH_BLOCK) tree_level_kernel(Op op, int first) {
  const int k = blockIdx.x * BVH_BLOCK + threadIdx.x;
  if (k < first) op.merge((int64_t)first + k);
}
// ---- the levels top .. 0 (top <= 8: at most 256 nodes) in one workgroup, and the unused node 0
template <class Op>
__global__ void __launch_bounds__(BVH_BLOCK) tree_top_kernel(Op op, int top) {
  for (int l = top; l >= 0; --l) {
    const int first = 1 << l;
    if ((int)threadIdx.x < first) op.merge((int64_t)first + threadIdx.x);
    __syncthreads();                                               // the level below is read from memory by other lanes
  }
  op.unused((int)threadIdx.x);
}

// The internal levels depth - 1 .. 0 behind the caller's launch of the leaves: one launch per level down to BVH_TOP_LEVELS, then
// one workgroup for the rest.
template <class Op>
int tree_reduce(const char* who_level, const char* who_top, Op op, int depth, hipStream_t st) {
  for (int l = depth - 1; l >= BVH_TOP_LEVELS; --l)
    DIST_LAUNCH(who_level, tree_level_kernel<Op>, blocks(bvh_level_nodes(l), BVH_BLOCK), op, (int)bvh_level_first(l));
  DIST_LAUNCH(who_top, tree_top_kernel<Op>, 1, op, (depth < BVH_TOP_LEVELS ? depth : BVH_TOP_LEVELS) - 1);
  return NERF_OK;
}

// each(f) for the valid sorted faces f of leaf `node` (P <= node < 2 P), in their order
template <class Each>
__device__ __forceinline__ void tree_leaf_faces(const int* __restrict__ order, int F, int P, uint32_t node, Each each) {
  const int s0 = BVH_LEAF * (int)(node - (uint32_t)P);
#pragma unroll
  for (int k = 0; k < BVH_LEAF; ++k) {
    const int f = s0 + k < F ? order[s0 + k] : -1;
    if (f >= 0) each(f);
  }
}

}  // namespace
}  // namespace nerf
