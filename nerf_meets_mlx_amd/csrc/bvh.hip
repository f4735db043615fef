// Mesh-to-mesh distance, the second face index: a bounding-volume hierarchy over the Morton-sorted faces, and the closest point of
// a given face.  Semantics in include/nerf_hip.h "mesh BVH"; tests/_bvh_ref.py reproduces every output bit for bit.  No reference
// counterpart.  The tree is a complete binary tree in heap order (bvh_ws.h), so that nothing here needs a workgroup to wait for
// another, a per-lane stack, a float atomic or a host read:
//   keys     one lane per face: the 36-bit Morton code of the midpoint of its bounding box, and the face number below it.  The
//            caller sorts the keys (they are unique: no sort order is left open).
//   leaves   one lane per leaf: the face ids of its four sorted keys (-1 for an invalid face) and the exact min / max of their
//            float32 corners.
//   level    one lane per node of a level: the union of its two children (bvh_tree.h's pass with BvhOp).  One launch per level; the
//            levels of at most 256 nodes share the last launch, one workgroup with a barrier between levels.
//   query    one lane per point: a stackless depth-first walk, the nearer child first; the lane keeps the node index and one
//            32-bit trail word with a bit per level where the far sibling is still pending.
//   closest  one lane per point: the region tests of distance.h on the given face, the computed q written out.
// Register use and what was measured: DESIGN.md section 38.
#include "bvh_tree.h"
#include "distance.h"

namespace nerf {
namespace {

struct BvhBox {
  double lo[3], ext[3];                                             // ext = (double)hi - (double)lo
  float box_abs;                                                    // the largest |corner coordinate|
};

// the Morton cell of the float64 coordinate m on an axis: clamp(floor((m - lo) / ext * 4096), 0, 4095)
__device__ __forceinline__ uint32_t bvh_cell(double m, double lo, double ext) {
  const double t = (m - lo) / ext * (double)BVH_CELLS;
  if (!(t > 0.0)) return 0u;
  if (t >= (double)BVH_CELLS) return (uint32_t)(BVH_CELLS - 1);
  return (uint32_t)t;
}
// the 12 bits of x spread to every third bit
__device__ __forceinline__ uint64_t bvh_spread(uint32_t x) {
  uint64_t v = x & 0xFFFu;
  v = (v | (v << 16)) & 0x00000000FF0000FFull;
  v = (v | (v << 8)) & 0x000000F00F00F00Full;
  v = (v | (v << 4)) & 0x00000030C30C30C3ull;
  v = (v | (v << 2)) & 0x0000009249249249ull;
  return v;
}

// ---- keys: 12 B of indices and 36 B of corners read per face, 8 B written
__global__ void __launch_bounds__(BVH_BLOCK) bvh_keys_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                            BvhBox bx, int64_t* __restrict__ keys) {
  const int f = blockIdx.x * BVH_BLOCK + threadIdx.x;
  if (f >= F) return;
  Tri t;
  float d;
  int64_t code = BVH_INVALID_CODE;
  if (dist_face(verts, faces, f, V, t, &d)) {
    uint64_t c = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double mn = (double)fminf(fminf(t.a[a], t.b[a]), t.c[a]), mx = (double)fmaxf(fmaxf(t.a[a], t.b[a]), t.c[a]);
      c |= bvh_spread(bvh_cell((mn + mx) * 0.5, bx.lo[a], bx.ext[a])) << a;
    }
    code = (int64_t)c;
  }
  keys[f] = code * ((int64_t)1 << BVH_KEY_SHIFT) + (int64_t)f;
}

__device__ __forceinline__ void bvh_store(float* __restrict__ nodes, int64_t i, const float* mn, const float* mx) {
  float* o = nodes + i * BVH_NODE_FLOATS;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    o[a] = mn[a];
    o[3 + a] = mx[a];
  }
}

// ---- leaves: one lane per leaf slot j in [0, P); 32 B of keys and four faces' corners read, 16 B of ids and 24 B of box written
__global__ void __launch_bounds__(BVH_BLOCK) bvh_leaves_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces,
                                                              int F, const int64_t* __restrict__ keys, int P,
                                                              float* __restrict__ nodes, int* __restrict__ order) {
  const int j = blockIdx.x * BVH_BLOCK + threadIdx.x;
  if (j >= P) return;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int k = 0; k < BVH_LEAF; ++k) {
    const int s = BVH_LEAF * j + k;
    if (s >= F) break;
    const int64_t key = keys[s];
    const int f = (int)(key & (((int64_t)1 << BVH_KEY_SHIFT) - 1));
    // a key is not trusted: the face is tested again, so that the query reads only through indices that are in range
    Tri t;
    float d;
    const bool ok = key >= 0 && (key >> BVH_KEY_SHIFT) < BVH_INVALID_CODE && f < F && dist_face(verts, faces, f, V, t, &d);
    order[s] = ok ? f : -1;
    if (!ok) continue;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = fminf(mn[a], fminf(fminf(t.a[a], t.b[a]), t.c[a]));
      mx[a] = fmaxf(mx[a], fmaxf(fmaxf(t.a[a], t.b[a]), t.c[a]));
    }
  }
  bvh_store(nodes, (int64_t)P + j, mn, mx);
}

// node i as the union of its children (an empty child is (+inf, -inf): the neutral element)
__device__ __forceinline__ void bvh_merge(float* nodes, int64_t i) {
  const float* l = nodes + 2 * i * BVH_NODE_FLOATS;
  float mn[3], mx[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    mn[a] = fminf(l[a], l[BVH_NODE_FLOATS + a]);
    mx[a] = fmaxf(l[3 + a], l[BVH_NODE_FLOATS + 3 + a]);
  }
  bvh_store(nodes, i, mn, mx);
}

// bvh_tree.h's Op: 48 B read and 24 B written per node; node 0 is an empty box
struct BvhOp {
  float* nodes;
  __device__ __forceinline__ void merge(int64_t i) const { bvh_merge(nodes, i); }
  __device__ __forceinline__ void unused(int lane) const {
    const float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (lane == 0) bvh_store(nodes, 0, mn, mx);
  }
};

// the squared float64 distance from p to the box (mn, mx); +inf for an empty box
__device__ __forceinline__ double bvh_box_d2(const double* p, float mn0, float mn1, float mn2, float mx0, float mx1, float mx2) {
  if (mn0 > mx0) return INFINITY;
  const double d0 = fmax(fmax((double)mn0 - p[0], p[0] - (double)mx0), 0.0);
  const double d1 = fmax(fmax((double)mn1 - p[1], p[1] - (double)mx1), 0.0);
  const double d2 = fmax(fmax((double)mn2 - p[2], p[2] - (double)mx2), 0.0);
  return (d0 * d0 + d1 * d1) + d2 * d2;
}

// The pruning rule: a node whose box is m = sqrt(m2) from the point is skipped only if it is empty or distance.h's dist_stop says
// so of m.  (m - slack)^2 (1 - 2^-20) < m^2, so m2 <= D never skips: the square root is taken only where it can matter.
__device__ __forceinline__ bool bvh_skip(double m2, double slack, uint64_t best) {
  if (m2 == INFINITY) return true;
  if (m2 <= (double)__uint_as_float((uint32_t)(best >> 32))) return false;
  return dist_stop(sqrt(m2), slack, best);
}

// ---- the query: 12 B read and 8 B written per point; per internal node visited 48 B of its children, per leaf 16 B of ids and per
// candidate 12 B of indices and 36 B of corners gathered.  No LDS, no scratch: no array here is indexed at run time.
__global__ void __launch_bounds__(BVH_BLOCK) bvh_query_kernel(const float* __restrict__ points, int64_t n, const float* __restrict__ verts,
                                                             const int* __restrict__ faces, int F, float box_abs, int P,
                                                             const float* __restrict__ nodes, const int* __restrict__ order,
                                                             float* __restrict__ dist2, int* __restrict__ face) {
  const int64_t i = (int64_t)blockIdx.x * BVH_BLOCK + threadIdx.x;
  if (i >= n) return;
  float p[3];
  if (!dist_point(points, i, p, [&] {
        dist2[i] = __uint_as_float(DIST_NAN32);
        face[i] = -1;
      }))
    return;
  const double pd[3] = {(double)p[0], (double)p[1], (double)p[2]};
  uint64_t best = DIST_NONE;
  const float* r = nodes + BVH_NODE_FLOATS;                          // the root, node 1
  const float r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4], r5 = r[5];
  if (r0 <= r3) {                                                    // a mesh with a valid face
    // the valid faces' largest |coordinate| is the root box's, which holds every corner
    const double slack = dist_slack(p, fmaxf(fmaxf(fmaxf(fabsf(r0), fabsf(r1)), fabsf(r2)), fmaxf(fmaxf(fabsf(r3), fabsf(r4)), fabsf(r5))),
                                    box_abs);
    uint32_t node = 1u, trail = 0u;                                  // trail bit j: the sibling of the ancestor j levels up is pending
    for (;;) {
      bool up = false;
      if (node >= (uint32_t)P) {                                     // a leaf: its valid faces into the minimum
        tree_leaf_faces(order, F, P, node, [&](int f) {
          Tri t;
          dist_load(verts, faces, f, t);
          best = dist_fold(best, point_triangle_d2(p, t), f);
        });
        up = true;
      } else {                                                       // the nearer child first, left on a tie
        const float4* c = reinterpret_cast<const float4*>(nodes + (size_t)2 * node * BVH_NODE_FLOATS);
        const float4 c0 = c[0], c1 = c[1], c2 = c[2];                // left (c0.xyz | c0.w c1.xy), right (c1.zw c2.x | c2.yzw)
        const double ml = bvh_box_d2(pd, c0.x, c0.y, c0.z, c0.w, c1.x, c1.y);
        const double mr = bvh_box_d2(pd, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w);
        const bool right = mr < ml;
        const bool near_ok = !bvh_skip(right ? mr : ml, slack, best), far_ok = !bvh_skip(right ? ml : mr, slack, best);
        const uint32_t nearer = 2u * node + (right ? 1u : 0u);
        if (near_ok) {
          node = nearer;
          trail = (trail << 1) | (far_ok ? 1u : 0u);
        } else if (far_ok) {
          node = nearer ^ 1u;
          trail <<= 1;
        } else {
          up = true;
        }
      }
      if (!up) continue;
      // pop to the lowest pending level; the sibling there is tested again, for the best may have improved since
      bool done = false;
      for (;;) {
        if (trail == 0u) {
          done = true;
          break;
        }
        const int k = __ffs((int)trail) - 1;
        trail = (trail >> k) & ~1u;
        node = (node >> k) ^ 1u;
        const float* b = nodes + (size_t)node * BVH_NODE_FLOATS;
        if (!bvh_skip(bvh_box_d2(pd, b[0], b[1], b[2], b[3], b[4], b[5]), slack, best)) break;
      }
      if (done) break;
    }
  }
  dist2[i] = __uint_as_float((uint32_t)(best >> 32));
  face[i] = (int)(uint32_t)(best & 0xFFFFFFFFull);
}

// ---- the closest point of a given face: 16 B read, 48 B gathered and 12 B written per point
__global__ void __launch_bounds__(BVH_BLOCK) bvh_closest_kernel(const float* __restrict__ points, int64_t n, const float* __restrict__ verts,
                                                               int V, const int* __restrict__ faces, int F, const int* __restrict__ face,
                                                               float* __restrict__ closest) {
  const int64_t i = (int64_t)blockIdx.x * BVH_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int f = face[i];
  const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
  float q[3] = {__uint_as_float(DIST_NAN32), __uint_as_float(DIST_NAN32), __uint_as_float(DIST_NAN32)};
  Tri t;
  float d;
  if (f >= 0 && f < F && dist_face(verts, faces, f, V, t, &d)) point_triangle_closest(p, t, q);
#pragma unroll
  for (int a = 0; a < 3; ++a) closest[3 * i + a] = q[a];
}

int bvh_box(const char* who, int64_t V, int64_t F, const float* lo, const float* hi, BvhBox* bx) {
  NERF_TRY(mesh_check(who, V, F));
  NERF_TRY(box_check(who, lo, hi));
  for (int a = 0; a < 3; ++a) {
    bx->lo[a] = (double)lo[a];
    bx->ext[a] = (double)hi[a] - (double)lo[a];
  }
  bx->box_abs = box_abs(lo, hi);
  return NERF_OK;
}

}  // namespace
}  // namespace nerf

using namespace nerf;

extern "C" int64_t nerf_bvh_workspace_bytes(int64_t F) { return bvh_workspace_bytes(F); }

extern "C" int nerf_bvh_keys(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* lo, const float* hi,
                             int64_t* keys, void* stream) {
  BvhBox bx;
  NERF_TRY(bvh_box("nerf_bvh_keys", V, F, lo, hi, &bx));
  if (F == 0) return NERF_OK;
  NERF_REQUIRE(faces && keys && (verts || V == 0), NERF_E_NULL, "nerf_bvh_keys: NULL pointer");
  hipStream_t st = as_stream(stream);
  DIST_LAUNCH("nerf_bvh_keys", bvh_keys_kernel, blocks(F, BVH_BLOCK), verts, (int)V, faces, (int)F, bx, keys);
  return NERF_OK;
}

extern "C" int nerf_bvh_build(const float* verts, int64_t V, const int32_t* faces, int64_t F, const int64_t* sorted_keys,
                              void* workspace, void* stream) {
  NERF_TRY(mesh_check("nerf_bvh_build", V, F));
  NERF_REQUIRE(workspace && (F == 0 || (faces && sorted_keys && verts)), NERF_E_NULL, "nerf_bvh_build: NULL pointer");
  NERF_TRY(ws_aligned16_check("nerf_bvh_build", workspace));
  const BvhWs w = bvh_ws(workspace, F);
  hipStream_t st = as_stream(stream);
  DIST_LAUNCH("nerf_bvh_build (leaves)", bvh_leaves_kernel, blocks(w.P, BVH_BLOCK), verts, (int)V, faces, (int)F, sorted_keys, (int)w.P, w.nodes,
             w.order);
  return tree_reduce("nerf_bvh_build (level)", "nerf_bvh_build (top)", BvhOp{w.nodes}, w.depth, st);
}

extern "C" int nerf_bvh_query(const float* points, int64_t n, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                              const float* lo, const float* hi, const void* workspace, float* dist2, int32_t* face, void* stream) {
  BvhBox bx;
  NERF_TRY(bvh_box("nerf_bvh_query", V, F, lo, hi, &bx));
  NERF_TRY(points_check("nerf_bvh_query", n));
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(points && workspace && dist2 && face && (F == 0 || (verts && faces)), NERF_E_NULL, "nerf_bvh_query: NULL pointer");
  NERF_TRY(ws_aligned16_check("nerf_bvh_query", workspace));
  const BvhWs w = bvh_ws(const_cast<void*>(workspace), F);
  hipStream_t st = as_stream(stream);
  DIST_LAUNCH("nerf_bvh_query", bvh_query_kernel, blocks(n, BVH_BLOCK), points, n, verts, faces, (int)F, bx.box_abs, (int)w.P,
             (const float*)w.nodes, (const int*)w.order, dist2, face);
  return NERF_OK;
}

extern "C" int nerf_closest_points(const float* points, int64_t n, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                                   const int32_t* face, float* closest, void* stream) {
  NERF_TRY(mesh_check("nerf_closest_points", V, F));
  NERF_TRY(points_check("nerf_closest_points", n));
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(points && face && closest && (F == 0 || faces) && (V == 0 || verts), NERF_E_NULL, "nerf_closest_points: NULL pointer");
  hipStream_t st = as_stream(stream);
  DIST_LAUNCH("nerf_closest_points", bvh_closest_kernel, blocks(n, BVH_BLOCK), points, n, verts, (int)V, faces, (int)F, face, closest);
  return NERF_OK;
}
