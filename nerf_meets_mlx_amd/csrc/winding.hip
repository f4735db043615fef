// The generalized winding number of a triangle mesh on the face hierarchy of bvh.hip: which side of an open, duplicated or
// self-intersecting mesh a point lies on.  Semantics in include/nerf_hip.h "mesh winding number"; tests/_winding_ref.py follows every
// operator.  No reference counterpart.  All arithmetic is float64 on the float32 corners and points, every operation rounded
// separately (-ffp-contract=off).  Nothing here needs a workgroup to wait for another, a per-lane stack, an atomic or a host read:
//   leaves   one lane per leaf: the area vectors, areas and area-weighted centroids of its valid faces, in sorted order.
//   level    one lane per node of a level: left + right, then the centre and the radius (bvh_tree.h's pass with WindOp: the
//            hierarchy's own launches).
//   query    one lane per point: a depth-first walk in heap order, left before right, that replaces a far subtree by its dipole.
//            The lane keeps the node index and nothing else; the order of the float64 sum is fixed by the tree.
// Register use and what was measured: DESIGN.md section 40.
#include "winding_ws.h"
#include "bvh_tree.h"
#include "distance.h"

namespace nerf {
namespace {

constexpr double WIND_FOUR_PI = 12.566370614359172;                 // 4 pi rounded to double

struct WindMom {
  double N[3], S[3], A;
};

__device__ __forceinline__ double wind_dot(const double* x, const double* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

// n_f = 0.5 (b - a) x (c - a), a_f = |n_f|; N += n_f, S += a_f ((a + b) + c) / 3, A += a_f
__device__ __forceinline__ void wind_add_face(WindMom& m, const Tri& t) {
  double e1[3], e2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    e1[k] = (double)t.b[k] - (double)t.a[k];
    e2[k] = (double)t.c[k] - (double)t.a[k];
  }
  const double n[3] = {0.5 * (e1[1] * e2[2] - e1[2] * e2[1]), 0.5 * (e1[2] * e2[0] - e1[0] * e2[2]), 0.5 * (e1[0] * e2[1] - e1[1] * e2[0])};
  const double af = sqrt(wind_dot(n, n));
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    m.N[k] += n[k];
    m.S[k] += (af * (((double)t.a[k] + (double)t.b[k]) + (double)t.c[k])) / 3.0;
  }
  m.A += af;
}

// the record of node i from its sums and its float32 box; zeros for an empty node
__device__ __forceinline__ void wind_store(double* mom, int64_t i, const WindMom& m, const float* box) {
  double* o = mom + i * WIND_NODE_DOUBLES;
  if (box[0] > box[3]) {
#pragma unroll
    for (int k = 0; k < WIND_NODE_DOUBLES; ++k) o[k] = 0.0;
    return;
  }
  double c[3], e[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double mn = (double)box[k], mx = (double)box[3 + k];
    c[k] = m.A == 0.0 ? (mn + mx) * 0.5 : m.S[k] / m.A;
    e[k] = fmax(c[k] - mn, mx - c[k]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[WIND_N + k] = m.N[k];
    o[WIND_C + k] = c[k];
    o[WIND_S + k] = m.S[k];
  }
  o[WIND_R] = sqrt(wind_dot(e, e));
  o[WIND_A] = m.A;
  o[WIND_S + 3] = 0.0;
}

// ---- leaves: one lane per leaf slot j in [0, P); 16 B of ids, 24 B of box and four faces' corners read, 96 B written
__global__ void __launch_bounds__(BVH_BLOCK) wind_leaves_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces,
                                                               int F, int P, const float* __restrict__ nodes,
                                                               const int* __restrict__ order, double* __restrict__ mom) {
  const int j = blockIdx.x * BVH_BLOCK + threadIdx.x;
  if (j >= P) return;
  WindMom m = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0.0};
#pragma unroll
  for (int k = 0; k < BVH_LEAF; ++k) {
    const int s = BVH_LEAF * j + k;
    const int f = s < F ? order[s] : -1;
    // the order is not trusted: the face is tested again, so that nothing is read through an index out of range
    Tri t;
    float d;
    if (f < 0 || f >= F || !dist_face(verts, faces, f, V, t, &d)) continue;
    wind_add_face(m, t);
  }
  const float* b = nodes + ((int64_t)P + j) * BVH_NODE_FLOATS;
  const float box[6] = {b[0], b[1], b[2], b[3], b[4], b[5]};
  wind_store(mom, (int64_t)P + j, m, box);
}

// node i as left + right, in that order
__device__ __forceinline__ void wind_merge(const float* nodes, double* mom, int64_t i) {
  const double* l = mom + 2 * i * WIND_NODE_DOUBLES;
  const double* r = l + WIND_NODE_DOUBLES;
  WindMom m;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    m.N[k] = l[WIND_N + k] + r[WIND_N + k];
    m.S[k] = l[WIND_S + k] + r[WIND_S + k];
  }
  m.A = l[WIND_A] + r[WIND_A];
  const float* b = nodes + i * BVH_NODE_FLOATS;
  const float box[6] = {b[0], b[1], b[2], b[3], b[4], b[5]};
  wind_store(mom, i, m, box);
}

// bvh_tree.h's Op: 192 B of records and 24 B of box read, 96 B written per node; node 0 is twelve zeros
struct WindOp {
  const float* nodes;
  double* mom;
  __device__ __forceinline__ void merge(int64_t i) const { wind_merge(nodes, mom, i); }
  __device__ __forceinline__ void unused(int lane) const { if (lane < WIND_NODE_DOUBLES) mom[lane] = 0.0; }
};

// the solid angle of the triangle seen from q: 2 atan2(det, den), 0 where q lies in its plane
__device__ __forceinline__ double wind_solid_angle(const double* q, const Tri& t) {
  double x[3], y[3], z[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    x[k] = (double)t.a[k] - q[k];
    y[k] = (double)t.b[k] - q[k];
    z[k] = (double)t.c[k] - q[k];
  }
  const double lx = sqrt(wind_dot(x, x)), ly = sqrt(wind_dot(y, y)), lz = sqrt(wind_dot(z, z));
  const double cr[3] = {y[1] * z[2] - y[2] * z[1], y[2] * z[0] - y[0] * z[2], y[0] * z[1] - y[1] * z[0]};
  const double det = wind_dot(x, cr);
  if (det == 0.0) return 0.0;
  const double den = (((lx * ly) * lz + wind_dot(x, y) * lz) + wind_dot(y, z) * lx) + wind_dot(z, x) * ly;
  return 2.0 * atan2(det, den);
}

// ---- the query: 12 B read and 16 B written per point; per node visited 8 B of its box, per internal node 56 B of its record, per
// leaf 16 B of ids and per face 12 B of indices and 36 B of corners gathered.  No LDS, no scratch: no array is indexed at run time.
__global__ void __launch_bounds__(BVH_BLOCK) wind_query_kernel(const float* __restrict__ points, int64_t n, const float* __restrict__ verts,
                                                              const int* __restrict__ faces, int F, int P,
                                                              const float* __restrict__ nodes, const int* __restrict__ order,
                                                              const double* __restrict__ mom, double beta2, double* __restrict__ w,
                                                              int* __restrict__ visits) {
  const int64_t i = (int64_t)blockIdx.x * BVH_BLOCK + threadIdx.x;
  if (i >= n) return;
  float p[3];
  if (!dist_point(points, i, p, [&] {
        w[i] = __longlong_as_double(DIST_NAN64);
        visits[2 * i] = 0;
        visits[2 * i + 1] = 0;
      }))
    return;
  const double q[3] = {(double)p[0], (double)p[1], (double)p[2]};
  double sum = 0.0;
  int exact = 0, approx = 0;
  uint32_t node = 1u;
  for (;;) {
    const float* b = nodes + (size_t)node * BVH_NODE_FLOATS;
    bool down = false;
    if (b[0] > b[3]) {                                               // an empty node: nothing below it
    } else if (node >= (uint32_t)P) {                                // a leaf: the exact term of each valid face
      tree_leaf_faces(order, F, P, node, [&](int f) {
        Tri t;
        dist_load(verts, faces, f, t);
        sum += wind_solid_angle(q, t);
        ++exact;
      });
    } else {                                                         // the dipole iff d^2 > beta^2 r^2, strictly
      const double* m = mom + (size_t)node * WIND_NODE_DOUBLES;
      const double d[3] = {m[WIND_C] - q[0], m[WIND_C + 1] - q[1], m[WIND_C + 2] - q[2]};
      const double d2 = wind_dot(d, d), r = m[WIND_R];
      if (d2 > beta2 * (r * r)) {
        const double N[3] = {m[WIND_N], m[WIND_N + 1], m[WIND_N + 2]};
        sum += wind_dot(N, d) / (d2 * sqrt(d2));
        ++approx;
      } else {
        down = true;
      }
    }
    if (down) {
      node = 2u * node;
      continue;
    }
    while (node & 1u) node >>= 1;                                    // next: up while a right child, then the right sibling
    if (node == 0u) break;
    node += 1u;
  }
  w[i] = sum / WIND_FOUR_PI;
  visits[2 * i] = exact;
  visits[2 * i + 1] = approx;
}

}  // namespace
}  // namespace nerf

using namespace nerf;

extern "C" int64_t nerf_winding_workspace_bytes(int64_t F) { return wind_workspace_bytes(F); }

extern "C" int nerf_winding_build(const float* verts, int64_t V, const int32_t* faces, int64_t F, const void* bvh_workspace,
                                  void* workspace, void* stream) {
  NERF_TRY(mesh_check("nerf_winding_build", V, F));
  if (F == 0) return NERF_OK;                                        // no face: the query finds the hierarchy's empty root
  NERF_REQUIRE(workspace && bvh_workspace && faces && verts, NERF_E_NULL, "nerf_winding_build: NULL pointer");
  NERF_TRY(ws_aligned16_check("nerf_winding_build", workspace, bvh_workspace));
  const BvhWs b = bvh_ws(const_cast<void*>(bvh_workspace), F);
  const WindWs w = wind_ws(workspace, F);
  hipStream_t st = as_stream(stream);
  DIST_LAUNCH("nerf_winding_build (leaves)", wind_leaves_kernel, blocks(w.P, BVH_BLOCK), verts, (int)V, faces, (int)F, (int)w.P,
              (const float*)b.nodes, (const int*)b.order, w.moments);
  return tree_reduce("nerf_winding_build (level)", "nerf_winding_build (top)", WindOp{b.nodes, w.moments}, w.depth, st);
}

extern "C" int nerf_winding_query(const float* points, int64_t n, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                                  const void* bvh_workspace, const void* workspace, double beta, double* w, int32_t* visits,
                                  void* stream) {
  NERF_TRY(mesh_check("nerf_winding_query", V, F));
  NERF_TRY(points_check("nerf_winding_query", n));
  NERF_REQUIRE(beta >= 1.0, NERF_E_SHAPE, "nerf_winding_query: need beta >= 1 or +inf (got %g)", beta);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(points && bvh_workspace && workspace && w && visits && (F == 0 || (verts && faces)), NERF_E_NULL,
               "nerf_winding_query: NULL pointer");
  NERF_TRY(ws_aligned16_check("nerf_winding_query", workspace, bvh_workspace));
  const BvhWs b = bvh_ws(const_cast<void*>(bvh_workspace), F);
  const WindWs m = wind_ws(const_cast<void*>(workspace), F);
  hipStream_t st = as_stream(stream);
  DIST_LAUNCH("nerf_winding_query", wind_query_kernel, blocks(n, BVH_BLOCK), points, n, verts, faces, (int)F, (int)m.P,
              (const float*)b.nodes, (const int*)b.order, (const double*)m.moments, beta * beta, w, visits);
  return NERF_OK;
}
