// What the point queries against a mesh share (distance.hip's grid, bvh.hip's hierarchy, winding.hip's moments on it): the face-validity
// rule, Ericson's point-triangle region tests, the 64-bit (distance, face) key, the load of a point, the stop rule of the two indices,
// the host checks and the launch.  Semantics in include/nerf_hip.h "mesh distance".  float32, every operation rounded separately (the
// units that include this build with -ffp-contract=off), the divisions correctly rounded; tests/_distance_ref.py reproduces every bit.
#pragma once
#include "lattice.h"

namespace nerf {
namespace {

constexpr int DIST_BLOCK = 256;                                    // lanes per workgroup of every kernel here (= BVH_BLOCK)
constexpr uint64_t DIST_NONE = 0x7F800000FFFFFFFFull;              // (+inf, face -1)
constexpr uint32_t DIST_NAN32 = 0x7FC00000u;                       // the quiet NaNs written where there is no answer
constexpr int64_t DIST_NAN64 = 0x7FF8000000000000ll;
constexpr int64_t MESH_MAX_POINTS = 1ll << 30;                     // points of a query, samples of a draw

__device__ __forceinline__ float dot3(const float* x, const float* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

struct Tri {
  float a[3], b[3], c[3];
};

// the corners of face f and its float32 doubled area; false for an invalid face (an index outside [0, V), a non-finite corner or
// a cross product that is exactly zero)
__device__ __forceinline__ bool dist_face(const float* __restrict__ verts, const int* __restrict__ faces, int f, int V, Tri& t,
                                          float* dbl_area) {
  int g[3];
  if (!mesh_corners(faces + 3 * f, V, g)) return false;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    t.a[k] = verts[3 * g[0] + k];
    t.b[k] = verts[3 * g[1] + k];
    t.c[k] = verts[3 * g[2] + k];
    ok = ok && isfinite(t.a[k]) && isfinite(t.b[k]) && isfinite(t.c[k]);
  }
  if (!ok) return false;
  float e1[3], e2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    e1[k] = t.b[k] - t.a[k];
    e2[k] = t.c[k] - t.a[k];
  }
  const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
  if (cx == 0.0f && cy == 0.0f && cz == 0.0f) return false;
  *dbl_area = sqrt_rn((cx * cx + cy * cy) + cz * cz);
  return true;
}

// the corners of a valid face (every index in range): no checks
__device__ __forceinline__ void dist_load(const float* __restrict__ verts, const int* __restrict__ faces, int f, Tri& t) {
  const int g0 = faces[3 * f], g1 = faces[3 * f + 1], g2 = faces[3 * f + 2];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    t.a[k] = verts[3 * g0 + k];
    t.b[k] = verts[3 * g1 + k];
    t.c[k] = verts[3 * g2 + k];
  }
}

// The closest point q of the triangle to p: Ericson, "Real-Time Collision Detection" 5.1.5, the region tests in his order; float32,
// every operation rounded separately, the divisions correctly rounded.  q is always a + v ab + w ac with v, w in [0, 1] as
// computed, so it lies within rounding of the triangle whatever region the rounded tests choose.
__device__ __forceinline__ void point_triangle_closest(const float* p, const Tri& t, float* q) {
  float ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ab[k] = t.b[k] - t.a[k];
    ac[k] = t.c[k] - t.a[k];
    ap[k] = p[k] - t.a[k];
    bp[k] = p[k] - t.b[k];
    cp[k] = p[k] - t.c[k];
  }
  const float d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float e43 = d4 - d3, e56 = d5 - d6;
  if (d1 <= 0.0f && d2 <= 0.0f) {                                   // vertex a
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = t.a[k];
  } else if (d3 >= 0.0f && d4 <= d3) {                              // vertex b
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = t.b[k];
  } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {              // edge ab
    const float v = div_rn(d1, d1 - d3);
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = t.a[k] + v * ab[k];
  } else if (d6 >= 0.0f && d5 <= d6) {                              // vertex c
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = t.c[k];
  } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {              // edge ac
    const float w = div_rn(d2, d2 - d6);
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = t.a[k] + w * ac[k];
  } else if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) {            // edge bc
    const float w = div_rn(e43, e43 + e56);
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = t.b[k] + w * (t.c[k] - t.b[k]);
  } else {                                                          // interior
    const float s = (va + vb) + vc;
    const float v = div_rn(vb, s), w = div_rn(vc, s);
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = (t.a[k] + v * ab[k]) + w * ac[k];
  }
}

// the squared distance from p to the triangle: dot(p - q, p - q)
__device__ __forceinline__ float point_triangle_d2(const float* p, const Tri& t) {
  float q[3];
  point_triangle_closest(p, t, q);
  const float d[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
  return dot3(d, d);
}

// the smaller of `best` and the key (bits of D) 2^32 + f of face f at squared distance d; a NaN distance never enters
__device__ __forceinline__ uint64_t dist_fold(uint64_t best, float d, int f) {
  if (d != d) return best;
  const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)f;
  return key < best ? key : best;
}

// Point i of points [n][3] into p; false, behind bad() writing the kernel's answer, when a coordinate is not finite.  (A callback
// keeps the three tests branches around it; returned as one plain bool they are evaluated together and the grid query takes 88 VGPRs.)
template <class Bad>
__device__ __forceinline__ bool dist_point(const float* __restrict__ points, int64_t i, float* p, Bad bad) {
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = points[3 * i + k];
  if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) return true;
  bad();
  return false;
}

// slack = S 2^-18, S the largest |coordinate| of the point, the valid faces and the box (why: distance.hip's query)
__device__ __forceinline__ double dist_slack(const float* p, float faces_max, float box_max) {
  const float S = fmaxf(fmaxf(fmaxf(fabsf(p[0]), fabsf(p[1])), fabsf(p[2])), fmaxf(faces_max, box_max));
  return (double)S * 0x1p-18;
}
// The stop rule of both indices.  Every face not yet seen is at least m from the point, so its float32 distance is at least
// (m - slack)^2 (1 - 2^-20): stop only when m > slack and that is strictly greater than the best D; on equality a lower face
// index may still tie.
__device__ __forceinline__ bool dist_stop(double m, double slack, uint64_t best) {
  const double s = m - slack;
  return s > 0.0 && (s * s) * (1.0 - 0x1p-20) > (double)__uint_as_float((uint32_t)(best >> 32));
}

// ---- host side: the checks of the query entries, each with its one text, and their launch
inline float box_abs(const float* lo, const float* hi) {           // the largest |corner coordinate|
  float m = 0.0f;
  for (int a = 0; a < 3; ++a) m = std::fmax(m, std::fmax(std::fabs(lo[a]), std::fabs(hi[a])));
  return m;
}
inline int points_check(const char* who, int64_t n) {
  NERF_REQUIRE(n >= 0 && n <= MESH_MAX_POINTS, NERF_E_SHAPE, "%s: need 0 <= n <= 2^30 (got %lld)", who, (long long)n);
  return NERF_OK;
}
inline bool ws_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int ws_aligned16_check(const char* who, const void* ws, const void* ws2 = nullptr) {
  NERF_REQUIRE(ws_aligned16(ws) && ws_aligned16(ws2), NERF_E_SHAPE, "%s: the workspace%s must start on a multiple of 16 bytes", who,
               ws2 ? "s" : "");
  return NERF_OK;
}
#define DIST_LAUNCH(what, kernel, blocks, ...) NERF_LAUNCH(what, kernel, blocks, DIST_BLOCK, st, __VA_ARGS__)

}  // namespace
}  // namespace nerf
