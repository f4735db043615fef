// Mesh-to-mesh distance: area-weighted surface sampling and closest-point queries against a uniform grid of faces.  Semantics in
// include/nerf_hip.h "mesh distance"; tests/_distance_ref.py reproduces every output bit for bit.  No reference counterpart.
//   cdf      one lane per face: the float32 doubled area as an integer weight -> int64 inclusive scan (count -> block scan -> write,
//            scan.h's single-workgroup pass between).  Exact, so independent of the summation order.
//   sample   one lane per sample: three counter-based draws, a binary search in the CDF, the point on the face.  No atomics.
//   count    one lane per face: one integer atomic per cell its clamped bounding box overlaps, and the largest |coordinate| of a
//            valid face (integer atomic max on the float's bits) -> exclusive scan of the cells.
//   fill     the face index through per-cell cursors.  The arrival order inside a cell is free: the query's minimum is a 64-bit
//            key (distance bits, face), which no order changes.
//   query    one lane per point: shells of cells by Chebyshev radius around the point's (clamped) cell until the bound says stop.
// Register use and what was measured: DESIGN.md section 37.
#include "distance.h"
#include "scan.h"

namespace nerf {
namespace {

constexpr int DIST_MAX_GRID = 256;                                 // G^3 <= 2^24 cells
constexpr int64_t DIST_MAX_ENTRIES = 1ll << 30;                    // offsets are ints
constexpr double DIST_W_LIM = 16.0, DIST_W_SCALE = 17179869184.0;  // weight = max(1, rint(min(d / U, 16) 2^34))

struct DistBox {
  double lo[3], h[3], inv[3];                                      // h = ext / G, inv = G / ext
  double unit;                                                     // U = the largest extent squared
  float box_abs;                                                   // the largest |corner coordinate|
  int G;
};

__host__ __device__ __forceinline__ uint64_t dist_mix64(uint64_t z) {      // splitmix64 finaliser, as occupancy.hip
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the integer weight of a valid face with doubled area d: at least 1; an overflowed (inf, NaN) area takes the cap
__device__ __forceinline__ int64_t dist_weight(float d, double unit) {
  double x = (double)d / unit;
  if (!(x < DIST_W_LIM)) x = DIST_W_LIM;
  const int64_t w = (int64_t)rint(x * DIST_W_SCALE);
  return w > 1 ? w : 1;
}

// the cell of coordinate x on axis a, clamped onto the grid (x finite)
__device__ __forceinline__ int dist_cell(const DistBox& bx, int a, float x) {
  const double t = ((double)x - bx.lo[a]) * bx.inv[a];
  if (!(t > 0.0)) return 0;
  if (t >= (double)bx.G) return bx.G - 1;
  return (int)t;
}

// ---- weights: 12 B of indices and 36 B of corners read per face, 8 B written; the workgroup's sum to blk
__global__ void __launch_bounds__(DIST_BLOCK) dist_weight_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces,
                                                                int F, double unit, int64_t* __restrict__ cdf,
                                                                int64_t* __restrict__ blk) {
  const int f = blockIdx.x * DIST_BLOCK + threadIdx.x;
  int64_t w = 0;
  if (f < F) {
    Tri t;
    float d;
    if (dist_face(verts, faces, f, V, t, &d)) w = dist_weight(d, unit);
    cdf[f] = w;
  }
  const int64_t s = block_sum<DIST_BLOCK, int64_t>(w);              // a weight does not fit an int
  if (threadIdx.x == 0) blk[blockIdx.x] = s;
}
// ---- weights -> inclusive CDF in place (every lane reads and writes its own element only)
__global__ void __launch_bounds__(DIST_BLOCK) dist_cdf_kernel(int64_t* __restrict__ cdf, int F, const int64_t* __restrict__ blk) {
  const int f = blockIdx.x * DIST_BLOCK + threadIdx.x;
  const int64_t v = f < F ? cdf[f] : 0;
  const int64_t c = block_offset<DIST_BLOCK, int64_t>(v, blk[blockIdx.x]) + v;
  if (f < F) cdf[f] = c;
}

// ---- samples: one lane each; log2(F) gathered CDF words, 12 + 36 B of the face, 16 B written
__global__ void __launch_bounds__(DIST_BLOCK) dist_sample_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                                const int64_t* __restrict__ cdf, uint64_t total, int64_t n,
                                                                uint64_t seed, float* __restrict__ points, int* __restrict__ face) {
  const int64_t i = (int64_t)blockIdx.x * DIST_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = dist_mix64(seed ^ dist_mix64((uint64_t)i + 0x632BE59BD9B4E019ull));
  const uint64_t r0 = dist_mix64(key + 1 * 0x9E3779B97F4A7C15ull), r1 = dist_mix64(key + 2 * 0x9E3779B97F4A7C15ull),
                 r2 = dist_mix64(key + 3 * 0x9E3779B97F4A7C15ull);
  const int64_t target = (int64_t)__umul64hi(r0, total);           // [0, total)
  int lo = 0, hi = F - 1;                                           // the first face whose inclusive CDF exceeds the target
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (cdf[mid] > target) hi = mid; else lo = mid + 1;
  }
  Tri t;
  float d;
  if (!dist_face(verts, faces, lo, V, t, &d)) {                     // only with a cdf or total that are not this mesh's
#pragma unroll
    for (int k = 0; k < 3; ++k) points[3 * i + k] = __uint_as_float(DIST_NAN32);
    face[i] = -1;
    return;
  }
  int a =(int)(r1 >> 40), b = (int)(r2 >> 40);                     // 24 bits each
  if (a + b > (1 << 24)) {                                          // u1 + u2 > 1: reflected across the diagonal
    a = (1 << 24) - a;
    b = (1 << 24) - b;
  }
  const float u1 = (float)a * 0x1p-24f, u2 = (float)b * 0x1p-24f;
#pragma unroll
  for (int k = 0; k < 3; ++k) points[3 * i + k] = (t.a[k] + u1 * (t.b[k] - t.a[k])) + u2 * (t.c[k] - t.a[k]);
  face[i] = lo;
}

// the cells [c0, c1] per axis that the clamped bounding box of a valid face overlaps
__device__ __forceinline__ void dist_span(const DistBox& bx, const Tri& t, int* c0, int* c1) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    c0[a] = dist_cell(bx, a, fminf(fminf(t.a[a], t.b[a]), t.c[a]));
    c1[a] = dist_cell(bx, a, fmaxf(fmaxf(t.a[a], t.b[a]), t.c[a]));
  }
}

// ---- entries per cell, and the largest |coordinate| of a valid face.  cnt and scale come in zeroed.
__global__ void __launch_bounds__(DIST_BLOCK) dist_count_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces,
                                                               int F, DistBox bx, int* __restrict__ cnt, uint32_t* __restrict__ scale) {
  const int f = blockIdx.x * DIST_BLOCK + threadIdx.x;
  Tri t;
  float d;
  if (f >= F || !dist_face(verts, faces, f, V, t, &d)) return;
  float m = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) m = fmaxf(m, fmaxf(fmaxf(fabsf(t.a[a]), fabsf(t.b[a])), fabsf(t.c[a])));
  atomicMax(scale, __float_as_uint(m));                             // non-negative floats order as their bits
  int c0[3], c1[3];
  dist_span(bx, t, c0, c1);
  for (int z = c0[2]; z <= c1[2]; ++z)
    for (int y = c0[1]; y <= c1[1]; ++y)
      for (int x = c0[0]; x <= c1[0]; ++x) atomicAdd(&cnt[x + bx.G * (y + bx.G * z)], 1);
}

// (cell offsets: scan.h's counts-to-offsets pair, clamped at DIST_MAX_ENTRIES -- a total beyond it is refused by the caller before
// anything reads the offsets -- with the total copied out)

// ---- entries: one cursor atomic and one 4-byte store per overlapped cell; nothing is written at or past E
__global__ void __launch_bounds__(DIST_BLOCK) dist_fill_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                              DistBox bx, int* __restrict__ cur, int* __restrict__ ent, int64_t E) {
  const int f = blockIdx.x * DIST_BLOCK + threadIdx.x;
  Tri t;
  float d;
  if (f >= F || !dist_face(verts, faces, f, V, t, &d)) return;
  int c0[3], c1[3];
  dist_span(bx, t, c0, c1);
  for (int z = c0[2]; z <= c1[2]; ++z)
    for (int y = c0[1]; y <= c1[1]; ++y)
      for (int x = c0[0]; x <= c1[0]; ++x) {
        const int slot = atomicAdd(&cur[x + bx.G * (y + bx.G * z)], 1);
        if (slot >= 0 && slot < E) ent[slot] = f;
      }
}

// ---- the query: 12 B read and 8 B written per point, and per candidate 12 B of indices and 36 B of corners gathered
__global__ void __launch_bounds__(DIST_BLOCK) dist_query_kernel(const float* __restrict__ points, int64_t n, const float* __restrict__ verts,
                                                               const int* __restrict__ faces, DistBox bx, const int* __restrict__ off,
                                                               const int* __restrict__ ent, int64_t E,
                                                               const uint32_t* __restrict__ scale, float* __restrict__ dist2,
                                                               int* __restrict__ face) {
  const int64_t i = (int64_t)blockIdx.x * DIST_BLOCK + threadIdx.x;
  if (i >= n) return;
  float p[3];
  if (!dist_point(points, i, p, [&] {
        dist2[i] = __uint_as_float(DIST_NAN32);
        face[i] = -1;
      }))
    return;
  const int G = bx.G;
  int c[3];
  double q[3];                                                       // the point projected onto the box
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    c[a] = dist_cell(bx, a, p[a]);
    q[a] = fmin(fmax((double)p[a], bx.lo[a]), bx.lo[a] + bx.h[a] * (double)G);
  }
  // The float32 distance of a face is that of a point within `slack` of the triangle (point_triangle_d2), taken with a relative
  // error below 2^-21: ten float32 operations on operands of at most 4 S each lead to the closest point and to the difference,
  // S the largest |coordinate| of the point, the valid faces and the box.  64 * 2^-24 S covers them and the double roundings of
  // the cell planes.
  const double slack = dist_slack(p, __uint_as_float(scale[0]), bx.box_abs);
  uint64_t best = DIST_NONE;
  for (int r = 0;; ++r) {
    const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, G - 1), y0 = max(c[1] - r, 0), y1 = min(c[1] + r, G - 1);
    const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, G - 1);
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        const bool whole = z == c[2] - r || z == c[2] + r || y == c[1] - r || y == c[1] + r;
        // a row on the shell's y or z faces is scanned whole; any other row only at its two ends x = cx - r, cx + r
        const int step = whole ? 1 : 2 * r;
        for (int x = whole ? x0 : c[0] - r; x <= (whole ? x1 : c[0] + r); x += step) {
          if (x < 0 || x >= G) continue;
          const int cell = x + G * (y + G * z);
          int e1 = off[cell + 1];
          if (e1 > E) e1 = (int)E;
          for (int e = off[cell]; e < e1; ++e) {
            const int f = ent[e];
            Tri t;
            dist_load(verts, faces, f, t);
            best = dist_fold(best, point_triangle_d2(p, t), f);
          }
        }
      }
    // The cells not yet visited lie beyond the six planes of the block [c - r, c + r]; m is the distance from q to the nearest of
    // those planes that has cells behind it.
    //  * Per-axis clamping of a face's bounding box only moves it nearer to a point inside the box, and a face is entered into
    //    every cell its clamped bounding box overlaps: for every point x of a face not yet seen, the projection of x onto the box
    //    lies in one of the face's cells, all of them unvisited, so |q - proj(x)| >= m.
    //  * Projection onto the box is non-expansive: |p - x| >= |q - proj(x)| >= m, for p inside the box (q = p) and outside.
    // So every unseen face has a true distance of at least m, which is what dist_stop asks for.
    double m = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (c[a] - r > 0) m = fmin(m, q[a] - (bx.lo[a] + bx.h[a] * (double)(c[a] - r)));
      if (c[a] + r + 1 < G) m = fmin(m, (bx.lo[a] + bx.h[a] * (double)(c[a] + r + 1)) - q[a]);
    }
    if (m == INFINITY) break;                                        // every cell has been visited
    if (dist_stop(m, slack, best)) break;
  }
  dist2[i] = __uint_as_float((uint32_t)(best >> 32));
  face[i] = (int)(uint32_t)(best & 0xFFFFFFFFull);
}

// ---- host side
struct DistWs {
  int64_t cells, nblk;
  int64_t* blk;                                      // [nblk] entries per workgroup of cells, scanned in place
  int64_t* total;                                    // [1]
  uint32_t* scale;                                   // [2] the bits of the largest |coordinate| of a valid face (8 B with padding)
  int32_t* off;                                      // [cells + 1]
  int32_t* cur;                                      // [cells]
  int64_t bytes;
};
inline bool dist_grid_ok(int G) { return G >= 1 && G <= DIST_MAX_GRID; }
inline DistWs dist_ws(void* ws, int G) {
  DistWs w;
  w.cells = (int64_t)G * G * G;
  w.nblk = mesh_blocks(w.cells, DIST_BLOCK);
  WsCarver<8> c(ws);
  w.blk = c.take<int64_t>(w.nblk);
  w.total = c.take<int64_t>(1);
  w.scale = c.take<uint32_t>(2);
  w.off = c.take<int32_t>(w.cells + 1);
  w.cur = c.take<int32_t>(w.cells);
  w.bytes = c.bytes();
  return w;
}

int dist_box(const char* who, int64_t V, int64_t F, const float* lo, const float* hi, int G, DistBox* bx) {
  NERF_TRY(mesh_check(who, V, F));
  NERF_REQUIRE(dist_grid_ok(G), NERF_E_SHAPE, "%s: need 1 <= grid <= %d (got %d)", who, DIST_MAX_GRID, G);
  NERF_TRY(box_check(who, lo, hi));
  double emax = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double ext = (double)hi[a] - (double)lo[a];
    bx->lo[a] = (double)lo[a];
    bx->h[a] = ext / (double)G;
    bx->inv[a] = (double)G / ext;
    emax = ext > emax ? ext : emax;
  }
  bx->unit = emax * emax;
  bx->box_abs = box_abs(lo, hi);
  bx->G = G;
  return NERF_OK;
}

}  // namespace
}  // namespace nerf

using namespace nerf;

extern "C" int64_t nerf_surface_cdf_workspace_bytes(int64_t F) {
  return F >= 0 && F <= MESH_MAX_ITEMS ? (blocks(F, DIST_BLOCK) + 1) * (int64_t)sizeof(int64_t) : -1;
}

extern "C" int nerf_surface_cdf(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* lo, const float* hi,
                                void* workspace, int64_t* cdf, void* stream) {
  DistBox bx;
  NERF_TRY(dist_box("nerf_surface_cdf", V, F, lo, hi, 1, &bx));
  if (F == 0) return NERF_OK;
  NERF_REQUIRE(faces && workspace && cdf && (verts || V == 0), NERF_E_NULL, "nerf_surface_cdf: NULL pointer");
  hipStream_t st = as_stream(stream);
  const int64_t nblk = blocks(F, DIST_BLOCK);
  int64_t* blk = static_cast<int64_t*>(workspace);
  DIST_LAUNCH("nerf_surface_cdf (weights)", dist_weight_kernel, nblk, verts, (int)V, faces, (int)F, bx.unit, cdf, blk);
  NERF_TRY(scan_launch("nerf_surface_cdf (scan)", blk, nblk, blk + nblk, st));
  DIST_LAUNCH("nerf_surface_cdf (write)", dist_cdf_kernel, nblk, cdf, (int)F, (const int64_t*)blk);
  return NERF_OK;
}

extern "C" int nerf_surface_sample(const float* verts, int64_t V, const int32_t* faces, int64_t F, const int64_t* cdf, int64_t total,
                                   int64_t n, uint64_t seed, float* points, int32_t* face, void* stream) {
  NERF_TRY(mesh_check("nerf_surface_sample", V, F));
  NERF_TRY(points_check("nerf_surface_sample", n));
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(total > 0 && F > 0, NERF_E_SHAPE, "nerf_surface_sample: the mesh has no area (total weight %lld over %lld faces)",
               (long long)total, (long long)F);
  NERF_REQUIRE(verts && faces && cdf && points && face, NERF_E_NULL, "nerf_surface_sample: NULL pointer");
  hipStream_t st = as_stream(stream);
  DIST_LAUNCH("nerf_surface_sample", dist_sample_kernel, blocks(n, DIST_BLOCK), verts, (int)V, faces, (int)F, cdf, (uint64_t)total, n, seed, points,
              face);
  return NERF_OK;
}

extern "C" int64_t nerf_meshdist_workspace_bytes(int64_t F, int grid) {
  return F >= 0 && F <= MESH_MAX_ITEMS && dist_grid_ok(grid) ? dist_ws(nullptr, grid).bytes : -1;
}

extern "C" int nerf_meshdist_count(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* lo, const float* hi,
                                   int grid, void* workspace, int64_t* total_out, void* stream) {
  DistBox bx;
  NERF_TRY(dist_box("nerf_meshdist_count", V, F, lo, hi, grid, &bx));
  NERF_REQUIRE(workspace && total_out && (faces || F == 0) && (verts || V == 0), NERF_E_NULL, "nerf_meshdist_count: NULL pointer");
  const DistWs w = dist_ws(workspace, grid);
  hipStream_t st = as_stream(stream);
  NERF_HIP("nerf_meshdist_count", hipMemsetAsync(w.cur, 0, w.cells * sizeof(int32_t), st));
  NERF_HIP("nerf_meshdist_count", hipMemsetAsync(w.scale, 0, 8, st));
  if (F > 0)
    DIST_LAUNCH("nerf_meshdist_count (count)", dist_count_kernel, blocks(F, DIST_BLOCK), verts, (int)V, faces, (int)F, bx, w.cur, w.scale);
  DIST_LAUNCH("nerf_meshdist_count (cell counts)", scan_offsets_count_kernel<DIST_BLOCK>, w.nblk, (const int*)w.cur, (int)w.cells, w.blk);
  NERF_TRY(scan_launch("nerf_meshdist_count (scan of the cells)", w.blk, w.nblk, w.total, st));
  DIST_LAUNCH("nerf_meshdist_count (cell offsets)", scan_offsets_write_kernel<DIST_BLOCK>, w.nblk, w.cur, (int)w.cells,
              (const int64_t*)w.blk, (const int64_t*)w.total, DIST_MAX_ENTRIES, w.off, total_out);
  return NERF_OK;
}

extern "C" int nerf_meshdist_build(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* lo, const float* hi,
                                   int grid, void* workspace, int32_t* entries, int64_t E, void* stream) {
  DistBox bx;
  NERF_TRY(dist_box("nerf_meshdist_build", V, F, lo, hi, grid, &bx));
  NERF_REQUIRE(E >= 0, NERF_E_SHAPE, "nerf_meshdist_build: need entries >= 0 (got %lld)", (long long)E);
  NERF_REQUIRE(E <= DIST_MAX_ENTRIES, NERF_E_SHAPE, "nerf_meshdist_build: %lld entries exceed 2^30; use a coarser grid", (long long)E);
  if (E == 0 || F == 0) return NERF_OK;
  NERF_REQUIRE(verts && faces && workspace && entries, NERF_E_NULL, "nerf_meshdist_build: NULL pointer");
  const DistWs w = dist_ws(workspace, grid);
  hipStream_t st = as_stream(stream);
  DIST_LAUNCH("nerf_meshdist_build (fill)", dist_fill_kernel, blocks(F, DIST_BLOCK), verts, (int)V, faces, (int)F, bx, w.cur, entries, E);
  return NERF_OK;
}

extern "C" int nerf_meshdist_query(const float* points, int64_t n, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                                   const float* lo, const float* hi, int grid, const void* workspace, const int32_t* entries, int64_t E,
                                   float* dist2, int32_t* face, void* stream) {
  DistBox bx;
  NERF_TRY(dist_box("nerf_meshdist_query", V, F, lo, hi, grid, &bx));
  NERF_TRY(points_check("nerf_meshdist_query", n));
  NERF_REQUIRE(E >= 0 && E <= DIST_MAX_ENTRIES, NERF_E_SHAPE, "nerf_meshdist_query: need 0 <= entries <= 2^30 (got %lld)", (long long)E);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(points && workspace && dist2 && face && (E == 0 || (verts && faces && entries)), NERF_E_NULL,
               "nerf_meshdist_query: NULL pointer");
  const DistWs w = dist_ws(const_cast<void*>(workspace), grid);
  hipStream_t st = as_stream(stream);
  DIST_LAUNCH("nerf_meshdist_query", dist_query_kernel, blocks(n, DIST_BLOCK), points, n, verts, faces, bx, (const int*)w.off, entries, E,
              (const uint32_t*)w.scale, dist2, face);
  return NERF_OK;
}
