// Taubin lambda|mu smoothing of a triangle mesh (G. Taubin, "A signal processing approach to fair surface design", 1995): the
// step between marching cubes and the simplifier.  Semantics in include/nerf_hip.h "mesh smoothing"; tests/_smooth_ref.py
// reproduces every output bit for bit.  No reference counterpart.  Store-then-sum: the adjacency is built once, every half-step
// gathers through it.
//   build    entries per vertex (one integer atomic per corner of a face) -> exclusive scan (count -> block scan -> write,
//            scan.h) -> the (b, c) entries through per-row cursors.  The arrival order inside a row is free: every sum that reads
//            a row is an exact integer sum.  No sort, no host read.
//   step     one lane per vertex: its row in 8-byte loads, two gathered neighbours per entry, 12 bytes written.  The caller's
//            output and one workspace buffer take turns so that the last half-step writes the output.  The fixed-point image of
//            a neighbour is recomputed at every reference: gathering a stored image (24 B instead of 12) measured slower, the
//            kernel is bound by its gathers and not by the double arithmetic.
//   normals  one lane per vertex over the same rows.
// All launch- or cache-bound.
#include "lattice.h"
#include "quadric.h"
#include "scan.h"
#include "smooth_ws.h"

namespace nerf {
namespace {

constexpr double SMOOTH_POS_LIM = 4.0, SMOOTH_POS_SCALE = 4294967296.0;        // fix(u, 4, 2^32)
constexpr double SMOOTH_NRM_LIM = 16.0, SMOOTH_NRM_SCALE = 17179869184.0;      // fix(c, 16, 2^34)
constexpr int SMOOTH_MAX_ITERATIONS = 1024;

struct SmoothBox {
  double c[3], ext[3];
};

// the three coordinates of vertex v as doubles; true when all are finite
__device__ __forceinline__ bool smooth_load(const float* __restrict__ verts, int v, double* x) {
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float f = verts[3 * v + a];
    x[a] = (double)f;
    ok = ok && isfinite(f);
  }
  return ok;
}

// the corners of face f; false for an ignored face (an index outside [0, V) or two equal corners)
__device__ __forceinline__ bool smooth_face(const int* __restrict__ faces, int f, int V, int* g) {
  return mesh_corners(faces + 3 * f, V, g) && mesh_distinct(g);
}

// ---- entries per vertex: 12 B read and three integer atomics per face.  cnt comes in zeroed.
__global__ void __launch_bounds__(SMOOTH_BLOCK) smooth_count_kernel(const int* __restrict__ faces, int F, int V, int* __restrict__ cnt) {
  const int f = blockIdx.x * SMOOTH_BLOCK + threadIdx.x;
  int g[3];
  if (f >= F || !smooth_face(faces, f, V, g)) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) atomicAdd(&cnt[g[c]], 1);
}

// (row offsets, entries per workgroup of 256 vertices and the row's first entry in off and in cur, the fill cursor: scan.h's
// counts-to-offsets pair.  At most 3 F <= 3 2^24 entries: no cap.)

// ---- entries: 12 B read per face, three cursor atomics, three 8-byte stores.  Row a receives (b, c), row b (c, a), row c (a, b).
__global__ void __launch_bounds__(SMOOTH_BLOCK) smooth_fill_kernel(const int* __restrict__ faces, int F, int V, int* __restrict__ cur,
                                                                  SmoothEntry* __restrict__ ent) {
  const int f = blockIdx.x * SMOOTH_BLOCK + threadIdx.x;
  int g[3];
  if (f >= F || !smooth_face(faces, f, V, g)) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int slot = atomicAdd(&cur[g[c]], 1);
    ent[slot] = SmoothEntry{g[(c + 1) % 3], g[(c + 2) % 3]};
  }
}

// ---- one half-step with factor k: per vertex 12 B + its row (8 B per entry) + two gathered positions per entry read, 12 B written
__global__ void __launch_bounds__(SMOOTH_BLOCK) smooth_step_kernel(const float* __restrict__ in, float* __restrict__ out, int V,
                                                                  const int* __restrict__ off, const SmoothEntry* __restrict__ ent,
                                                                  SmoothBox bx, double k) {
  const int v = blockIdx.x * SMOOTH_BLOCK + threadIdx.x;
  if (v >= V) return;
  const float own[3] = {in[3 * v], in[3 * v + 1], in[3 * v + 2]};
  int64_t S[3] = {0, 0, 0};
  int n = 0;
  if (isfinite(own[0]) && isfinite(own[1]) && isfinite(own[2])) {
    const int e1 = off[v + 1];
    for (int e = off[v]; e < e1; ++e) {
      const SmoothEntry t = ent[e];
      const int nb[2] = {t.b, t.c};
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        double y[3];
        if (!smooth_load(in, nb[j], y)) continue;
        ++n;
#pragma unroll
        for (int a = 0; a < 3; ++a) S[a] += fixed((y[a] - bx.c[a]) / bx.ext[a], SMOOTH_POS_LIM, SMOOTH_POS_SCALE);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float o = own[a];                                // n = 0 (a non-finite vertex of its own included): the bits are copied
    if (n > 0) {
      const double x = (double)own[a];
      const double mean = bx.c[a] + ((double)S[a] / SMOOTH_POS_SCALE / (double)n) * bx.ext[a];
      o = (float)(x + k * (mean - x));
    }
    out[3 * v + a] = o;
  }
}

// ---- normals: the area-weighted sum of the face normals around a vertex, in box units, as exact integers
__global__ void __launch_bounds__(SMOOTH_BLOCK) smooth_normals_kernel(const float* __restrict__ verts, int V, const int* __restrict__ off,
                                                                     const SmoothEntry* __restrict__ ent, SmoothBox bx,
                                                                     float* __restrict__ normals, float* __restrict__ rows) {
  const int v = blockIdx.x * SMOOTH_BLOCK + threadIdx.x;
  if (v >= V) return;
  double x[3];
  int64_t N[3] = {0, 0, 0};
  if (smooth_load(verts, v, x)) {
    const int e1 = off[v + 1];
    for (int e = off[v]; e < e1; ++e) {
      const SmoothEntry t = ent[e];
      double yb[3], yc[3];
      const bool okb = smooth_load(verts, t.b, yb), okc = smooth_load(verts, t.c, yc);
      if (!okb || !okc) continue;
      double d1[3], d2[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        d1[a] = (yb[a] - x[a]) / bx.ext[a];
        d2[a] = (yc[a] - x[a]) / bx.ext[a];
      }
      N[0] += fixed(d1[1] * d2[2] - d1[2] * d2[1], SMOOTH_NRM_LIM, SMOOTH_NRM_SCALE);
      N[1] += fixed(d1[2] * d2[0] - d1[0] * d2[2], SMOOTH_NRM_LIM, SMOOTH_NRM_SCALE);
      N[2] += fixed(d1[0] * d2[1] - d1[1] * d2[0], SMOOTH_NRM_LIM, SMOOTH_NRM_SCALE);
    }
  }
  const double s[3] = {((double)N[0] / SMOOTH_NRM_SCALE) * (bx.ext[1] * bx.ext[2]), ((double)N[1] / SMOOTH_NRM_SCALE) * (bx.ext[2] * bx.ext[0]),
                       ((double)N[2] / SMOOTH_NRM_SCALE) * (bx.ext[0] * bx.ext[1])};
  const double len = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
  float xo[3], no[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    xo[a] = verts[3 * v + a];
    no[a] = len > 0.0 ? (float)(s[a] / len) : 0.0f;
    normals[3 * v + a] = no[a];
  }
  if (rows) write_color_row(rows, v, xo, no);
}

int smooth_box(const char* who, int64_t V, const float* lo, const float* hi, SmoothBox* bx) {
  NERF_REQUIRE(V >= 0 && V <= MESH_MAX_ITEMS, NERF_E_SHAPE, "%s: need 0 <= V <= 2^24 (got %lld)", who, (long long)V);
  NERF_TRY(box_check(who, lo, hi));
  for (int a = 0; a < 3; ++a) {
    bx->ext[a] = (double)hi[a] - (double)lo[a];
    bx->c[a] = ((double)lo[a] + (double)hi[a]) * 0.5;
  }
  return NERF_OK;
}

#define SMOOTH_LAUNCH(what, kernel, blocks, ...) NERF_LAUNCH(what, kernel, blocks, SMOOTH_BLOCK, st, __VA_ARGS__)

}  // namespace
}  // namespace nerf

using namespace nerf;

extern "C" int64_t nerf_smooth_workspace_bytes(int64_t V, int64_t F) { return smooth_workspace_bytes(V, F); }

extern "C" int nerf_smooth_build(int64_t V, const int32_t* faces, int64_t F, void* workspace, void* stream) {
  NERF_REQUIRE(smooth_sizes_ok(V, F), NERF_E_SHAPE, "nerf_smooth_build: need 0 <= V, F <= 2^24 (got %lld, %lld)", (long long)V,
               (long long)F);
  if (V == 0) return NERF_OK;
  NERF_REQUIRE(workspace && (faces || F == 0), NERF_E_NULL, "nerf_smooth_build: NULL pointer");
  const SmoothWs w = smooth_ws(workspace, V, F);
  hipStream_t st = as_stream(stream);
  // F = 0: every row is empty, and the zeroed offsets say so; nothing is launched
  NERF_HIP("nerf_smooth_build", F == 0 ? hipMemsetAsync(w.off, 0, (V + 1) * sizeof(int32_t), st)
                                       : hipMemsetAsync(w.cur, 0, V * sizeof(int32_t), st));
  if (F == 0) return NERF_OK;
  const int64_t nblk_f = mesh_blocks(F, SMOOTH_BLOCK);
  SMOOTH_LAUNCH("nerf_smooth_build (count)", smooth_count_kernel, nblk_f, faces, (int)F, (int)V, w.cur);
  SMOOTH_LAUNCH("nerf_smooth_build (row counts)", scan_offsets_count_kernel<SMOOTH_BLOCK>, w.nblk_v, (const int*)w.cur, (int)V, w.blk);
  NERF_TRY(scan_launch("nerf_smooth_build (scan of the rows)", w.blk, w.nblk_v, w.total, st));
  SMOOTH_LAUNCH("nerf_smooth_build (row offsets)", scan_offsets_write_kernel<SMOOTH_BLOCK>, w.nblk_v, w.cur, (int)V,
                (const int64_t*)w.blk, (const int64_t*)w.total, (int64_t)INT64_MAX, w.off, (int64_t*)nullptr);
  SMOOTH_LAUNCH("nerf_smooth_build (fill)", smooth_fill_kernel, nblk_f, faces, (int)F, (int)V, w.cur, w.ent);
  return NERF_OK;
}

extern "C" int nerf_smooth_run(const float* verts_in, int64_t V, const float* lo, const float* hi, int iterations, float lambda,
                               float mu, void* workspace, float* verts_out, void* stream) {
  SmoothBox bx;
  NERF_TRY(smooth_box("nerf_smooth_run", V, lo, hi, &bx));
  NERF_REQUIRE(iterations >= 1 && iterations <= SMOOTH_MAX_ITERATIONS, NERF_E_SHAPE, "nerf_smooth_run: need 1 <= iterations <= %d (got %d)",
               SMOOTH_MAX_ITERATIONS, iterations);
  NERF_REQUIRE(lambda > 0.0f && lambda <= 1.0f, NERF_E_SHAPE, "nerf_smooth_run: need 0 < lambda <= 1 (got %g)", (double)lambda);
  NERF_REQUIRE(mu == 0.0f || (mu >= -2.0f && mu < 0.0f), NERF_E_SHAPE, "nerf_smooth_run: need mu = 0 or -2 <= mu < 0 (got %g)", (double)mu);
  if (V == 0) return NERF_OK;
  NERF_REQUIRE(verts_in && workspace && verts_out, NERF_E_NULL, "nerf_smooth_run: NULL pointer");
  // the F of the build call only sizes the entries, the workspace's last region
  const SmoothWs w = smooth_ws(workspace, V, 0);
  hipStream_t st = as_stream(stream);
  const int per = mu == 0.0f ? 1 : 2, steps = iterations * per;
  const float* src = verts_in;
  for (int j = 0; j < steps; ++j) {
    float* dst = ((steps - 1 - j) & 1) ? w.tmp : verts_out;        // the last half-step lands in the output
    const double k = (double)((per == 2 && (j & 1)) ? mu : lambda);
    SMOOTH_LAUNCH("nerf_smooth_run (half-step)", smooth_step_kernel, w.nblk_v, src, dst, (int)V, (const int*)w.off,
                  (const SmoothEntry*)w.ent, bx, k);
    src = dst;
  }
  return NERF_OK;
}

extern "C" int nerf_smooth_normals(const float* verts, int64_t V, const float* lo, const float* hi, void* workspace, float* normals_out,
                                   float* color_rows, void* stream) {
  SmoothBox bx;
  NERF_TRY(smooth_box("nerf_smooth_normals", V, lo, hi, &bx));
  if (V == 0) return NERF_OK;
  NERF_REQUIRE(verts && workspace && normals_out, NERF_E_NULL, "nerf_smooth_normals: NULL pointer");
  const SmoothWs w = smooth_ws(workspace, V, 0);
  hipStream_t st = as_stream(stream);
  SMOOTH_LAUNCH("nerf_smooth_normals", smooth_normals_kernel, w.nblk_v, verts, (int)V, (const int*)w.off, (const SmoothEntry*)w.ent, bx,
                normals_out, color_rows);
  return NERF_OK;
}
