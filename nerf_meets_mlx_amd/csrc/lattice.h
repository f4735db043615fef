// The lattice of the volume kernels (mesh.hip, ccl.hip, morph.hip, tsdf.hip; simplify.hip for the checks and the colour row), the
// one statement in code of include/nerf_hip.h "mesh extraction":
//   volume   contiguous float32 [R, R, R], linear index p = i + R (j + R k), 2 <= R <= NERF_MESH_MAX_RES, so R^3 <= 2^27 fits an int;
//            inside means v > iso, iso finite
//   box      finite lo_a < hi_a, h_a = (hi_a - lo_a) / R in float32 with two roundings (the subtraction, then the division)
//   centres  p_a = lo_a + ((float)i_a + 0.5f) h_a, a multiply and an add rounded separately (-ffp-contract=off)
//   launch   one lane per voxel, x fastest, LATTICE_BLOCK voxels per workgroup
// The index helpers compile without HIP (tests/lattice_check.cpp runs them under a host compiler, which supplies nerf::fail and
// NERF_REQUIRE itself).  Not here, on purpose: simplify.hip's double-precision SBox (another lattice, of G^3 cells), morph.hip's
// word geometry (it counts 64-voxel words) and ccl.hip's union-find.
// Below the lattice, the triangle mesh as the surface kernels take it (texture.hip, raster.hip, project.hip, mip.hip; smooth.hip for
// the corners): verts float32 [V, 3], faces int32 [F, 3], 0 <= V, F <= MESH_MAX_ITEMS (mesh_ws.h), nothing read through an index
// outside [0, V).  Not simplify.hip's checks (one message for V and F) or its fetch, which tests only >= 0.
#pragma once
#include <cmath>
#include <stdint.h>
#include "mesh_ws.h"
#if defined(__HIPCC__)
#include "common.h"
#else
#include "../../include/nerf_hip.h"
#if !defined(__host__)
#define __host__
#define __device__
#define __forceinline__ inline
#endif
#endif

namespace nerf {
namespace {

constexpr int LATTICE_BLOCK = 256;                  // voxels per workgroup, x fastest

struct Lattice {
  int R;
  float lo[3], h[3];
};

__host__ __device__ __forceinline__ int64_t lattice_n3(int R) { return (int64_t)R * R * R; }
__host__ __device__ __forceinline__ void lattice_coords(int l, int R, int* c) { c[0] = l % R; c[1] = (l / R) % R; c[2] = l / (R * R); }
__host__ __device__ __forceinline__ void lattice_centre(const Lattice& lat, const int* c, float* p) {
#pragma unroll
  for (int a = 0; a < 3; ++a) p[a] = lat.lo[a] + ((float)c[a] + 0.5f) * lat.h[a];
}
__host__ __device__ __forceinline__ int axis_stride(int a, int R) { return a == 0 ? 1 : (a == 1 ? R : R * R); }
inline unsigned lattice_blocks(int R) { return (unsigned)((lattice_n3(R) + LATTICE_BLOCK - 1) / LATTICE_BLOCK); }

inline bool lattice_res_ok(int R) { return R >= 2 && R <= NERF_MESH_MAX_RES; }      // (the *_workspace_bytes: no error text)
// `name`: what the entry calls its R in the error text ("res"; the simplifier's "grid")
inline int lattice_res_check(const char* who, int R, const char* name = "res") {
  NERF_REQUIRE(lattice_res_ok(R), NERF_E_SHAPE, "%s: need 2 <= %s <= %d (got %d)", who, name, NERF_MESH_MAX_RES, R);
  return NERF_OK;
}
inline int lattice_check(const char* who, int R, float iso) {
  const int rc = lattice_res_check(who, R);
  if (rc) return rc;
  NERF_REQUIRE(std::isfinite(iso), NERF_E_SHAPE, "%s: iso must be finite", who);
  return NERF_OK;
}
inline int box_check(const char* who, const float* lo, const float* hi) {
  NERF_REQUIRE(lo && hi, NERF_E_NULL, "%s: NULL lo / hi", who);
  for (int a = 0; a < 3; ++a)
    NERF_REQUIRE(std::isfinite(lo[a]) && std::isfinite(hi[a]) && lo[a] < hi[a], NERF_E_SHAPE,
                 "%s: need finite lo[%d] < hi[%d] (got %g, %g)", who, a, a, (double)lo[a], (double)hi[a]);
  return NERF_OK;
}
inline int lattice_box(const char* who, int R, const float* lo, const float* hi, Lattice* lat) {
  const int rc = box_check(who, lo, hi);
  if (rc) return rc;
  lat->R = R;
  for (int a = 0; a < 3; ++a) {
    lat->lo[a] = lo[a];
    lat->h[a] = (hi[a] - lo[a]) / (float)R;                // float32, two roundings
    NERF_REQUIRE(lat->h[a] > 0.0f && std::isfinite(lat->h[a]), NERF_E_SHAPE, "%s: box too small or too large on axis %d", who, a);
  }
  return NERF_OK;
}

inline int mesh_check(const char* who, int64_t V, int64_t F) {             // (an entry without vertices passes V = 0)
  NERF_REQUIRE(V >= 0 && V <= MESH_MAX_ITEMS, NERF_E_SHAPE, "%s: need 0 <= V <= 2^24 (got %lld)", who, (long long)V);
  NERF_REQUIRE(F >= 0 && F <= MESH_MAX_ITEMS, NERF_E_SHAPE, "%s: need 0 <= F <= 2^24 (got %lld)", who, (long long)F);
  return NERF_OK;
}
// the corners g of the face whose three indices start at idx; false when one lies outside [0, V)
__host__ __device__ __forceinline__ bool mesh_corners(const int* __restrict__ idx, int V, int* g) {
  g[0] = idx[0], g[1] = idx[1], g[2] = idx[2];
  return g[0] >= 0 && g[0] < V && g[1] >= 0 && g[1] < V && g[2] >= 0 && g[2] < V;
}
// no two of the three corners are one vertex (smooth.hip and decimate.hip ignore a face that fails this)
__host__ __device__ __forceinline__ bool mesh_distinct(const int* g) { return g[0] != g[1] && g[1] != g[2] && g[0] != g[2]; }

// correctly rounded float32 division / square root: the double result rounded once (exact enough for one float rounding)
__host__ __device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }
__host__ __device__ __forceinline__ float sqrt_rn(float a) { return (float)sqrt((double)a); }

#if defined(__HIPCC__)
// this lane's voxel; at or past lattice_n3(R) in the last workgroup's tail
__device__ __forceinline__ int64_t lattice_lane() { return (int64_t)blockIdx.x * LATTICE_BLOCK + threadIdx.x; }

// the colour query row [x, -n, 0, 0, -n] of vertex `id`
__device__ __forceinline__ void write_color_row(float* __restrict__ rows, int64_t id, const float* x, const float* n) {
  float* r = rows + id * NERF_RAY_STRIDE;
#pragma unroll
  for (int a = 0; a < 3; ++a) { r[a] = x[a]; r[3 + a] = -n[a]; r[8 + a] = -n[a]; }
  r[6] = 0.0f; r[7] = 0.0f;
}
#endif

inline uint32_t float_bits(float x) {
  uint32_t b;
  static_assert(sizeof(b) == sizeof(x), "float32");
  __builtin_memcpy(&b, &x, sizeof(b));
  return b;
}

}  // namespace
}  // namespace nerf
